"""Shared by tests/test_assemble_host.py, tests/test_gpu_assemble.py, tests/hooks_assemble_check.py, tools/fuzz_assemble.py
and tools/assemble_bench.py: builds and runs the CPU model (tests/cpp/assemble_model.cc) and makes the drives -- synthetic
scans in the SENSOR frame with the scan model's per-point relative times, against the corkscrew sampled as a trajectory."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "assemble_model.cc")
LOOKUP, ASSEMBLE = 1, 2
TICKS = 10_000_000  # common::Time ticks (100 ns) a second
EPOCH = 636_000_000_000_000_000  # a universal time of 2016: such ticks need 60 bits, more than a double's 53
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
# sensor_to_tracking of the drives: a lidar mounted off the tracking frame's origin and tilted, and the same without the offset
MOUNT = np.array([0.21, -0.04, 0.37, 0.9887710779360422, 0.0, 0.1494381324735992, 0.0])
MOUNT_NO_TRANSLATION = np.concatenate([np.zeros(3), MOUNT[3:]])
f32 = np.float32


def build_model(directory):
    exe = os.path.join(str(directory), "assemble_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def ticks(seconds):
    return EPOCH + int(round(float(seconds) * TICKS))


def lookup_op(times):
    return (LOOKUP, np.ascontiguousarray(times, dtype=np.int64).reshape(-1))


def assemble_op(cloud_time, sensor_to_tracking, xyzt):
    return (ASSEMBLE, int(cloud_time), np.ascontiguousarray(sensor_to_tracking, dtype=np.float64).reshape(7),
            np.ascontiguousarray(xyzt, dtype=f32).reshape(-1, 4))


def run_model(exe, times, poses, ops, directory, timing=False):
    """-> (status of the pushes, results[, stdout]): per lookup op (has bool[k], poses float64 (k, 7)), per assemble op a
    dict status / index / xyz / origin / libm / intervals."""
    src, dst = os.path.join(str(directory), "assemble_ops.bin"), os.path.join(str(directory), "assemble_out.bin")
    times = np.ascontiguousarray(times, dtype=np.int64).reshape(-1)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(times)))
        f.write(times.tobytes())
        f.write(poses.tobytes())
        for o in ops:
            if o[0] == LOOKUP:
                f.write(struct.pack("<iq", LOOKUP, len(o[1])))
                f.write(o[1].tobytes())
            else:
                f.write(struct.pack("<iq", ASSEMBLE, o[1]))
                f.write(o[2].tobytes())
                f.write(struct.pack("<q", len(o[3])))
                f.write(o[3].tobytes())
    text = subprocess.check_output([exe, src, dst] + (["--time"] if timing else [])).decode()
    data = open(dst, "rb").read()
    pushed = struct.unpack_from("<i", data, 0)[0]
    at, results = 4, []
    if pushed == 0:
        for o in ops:
            if o[0] == LOOKUP:
                rows = np.frombuffer(data, dtype=np.dtype([("has", "<i4"), ("pose", "<f8", 7)]), count=len(o[1]), offset=at)
                at += 60 * len(o[1])
                results.append((rows["has"] != 0, rows["pose"].copy()))
                continue
            status, kept = struct.unpack_from("<iq", data, at)
            at += 12
            index = np.frombuffer(data, dtype=np.int32, count=kept, offset=at).copy()
            at += 4 * kept
            xyz = np.frombuffer(data, dtype=f32, count=3 * kept, offset=at).reshape(kept, 3).copy()
            at += 12 * kept
            origin = np.frombuffer(data, dtype=f32, count=3, offset=at).copy()
            libm, intervals = struct.unpack_from("<qq", data, at + 12)
            at += 28
            results.append(dict(status=status, index=index, xyz=xyz, origin=origin, libm=libm, intervals=intervals))
        assert at == len(data)
    return (pushed, results, text) if timing else (pushed, results)


def corkscrew(nodes, span, t0=0.3):
    """`nodes` nodes of the corkscrew, evenly over `span` seconds from t0 -> (ticks int64[nodes], poses float64 (nodes, 7))."""
    from dliom import synth
    at = t0 + span * np.arange(nodes) / max(nodes - 1, 1)
    return np.array([ticks(t) for t in at], dtype=np.int64), np.array([synth.trajectory_pose(t) for t in at])


# nodes -> seconds they span: 200 Hz for the long ones (a 0.1 s scan crosses 20 intervals), and two short ones that a scan
# overhangs at both ends
SPANS = {2: 0.08, 3: 0.09, 37: 0.18, 200: 0.995}


def drive(beams, azimuths, nodes):
    """A scan swept while the sensor flies the corkscrew, in the sensor frame, its 0.1 s centred on a trajectory of `nodes`
    nodes -> (times, poses, cloud_time, xyzt float32 (n, 4))."""
    from dliom import synth
    span = SPANS[nodes]
    times, poses = corkscrew(nodes, span)
    t_end = 0.3 + 0.5 * span + 0.05
    return times, poses, ticks(t_end), synth.moving_scan(t_end, beams, azimuths)


def honest(result, nodes):
    """The conditions under which a drive compares something: the scan crosses at least three intervals (every interval of
    a trajectory that has fewer), and at least 90 % of the kept points take slerp's sin / acos branch."""
    assert result["status"] == 0
    kept = len(result["index"])
    assert kept > 0
    assert result["intervals"] >= min(3, nodes - 1), result["intervals"]
    assert result["libm"] >= 0.9 * kept, (result["libm"], kept)
    return kept


def random_quaternion(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def random_case(seed):
    """A randomised trajectory and batch -> (times, poses, cloud_time, sensor_to_tracking, xyzt): 1..60 nodes with gaps of
    0 (duplicated times) to 50 ms, rotations that move a little, a lot, not at all or to the other sign of the quaternion,
    1..3000 points whose times overhang the trajectory at both ends, some of them exactly on node times."""
    from dliom import synth
    rng = np.random.RandomState(seed)
    nodes = int(rng.randint(1, 61))
    gaps = rng.randint(1, 500_000, size=nodes)
    gaps[rng.uniform(size=nodes) < 0.1] = 0
    times = EPOCH + int(rng.randint(0, 10**9)) + np.cumsum(gaps).astype(np.int64)
    poses = np.zeros((nodes, 7))
    q = random_quaternion(rng)
    p = rng.uniform(-50.0, 50.0, size=3)
    for i in range(nodes):
        kind = rng.randint(0, 6)
        if kind == 0:
            q = random_quaternion(rng)  # a large step, any sign of the dot product
        elif kind == 1:
            q = -q  # the same rotation, d = -1
        elif kind != 2:  # (2: the identical rotation, the absD >= one branch)
            step = synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.2))
            q = synth.quat_mul(q, step)
            q = q / np.linalg.norm(q)
            if rng.uniform() < 0.2:
                q = -q
        p = p + rng.uniform(-0.3, 0.3, size=3)
        poses[i] = np.concatenate([p, q])
    n = int(rng.randint(1, 3001))
    cloud_time = int(times[-1]) + int(rng.randint(-100_000, 100_000))
    reach = (int(times[-1]) - int(times[0]) + 400_000) / TICKS
    xyzt = np.zeros((n, 4), dtype=f32)
    xyzt[:, :3] = rng.uniform(-30.0, 30.0, size=(n, 3))
    xyzt[:, 3] = rng.uniform(-reach, 0.02, size=n)
    on_node = rng.randint(0, nodes, size=max(n // 50, 1))  # (where the float holds the offset exactly, the point is on the node)
    xyzt[:len(on_node), 3] = ((times[on_node] - cloud_time) / TICKS).astype(f32)
    mount = IDENTITY.copy() if rng.uniform() < 0.25 else np.concatenate([rng.uniform(-1.0, 1.0, size=3), random_quaternion(rng)])
    if rng.uniform() < 0.3:
        mount[:3] = 0.0
    return times, poses, cloud_time, mount, xyzt


def assert_equal_bits(cloud, origin, index, want):
    """A device result (dliom.Trajectory.assemble) against the model's: indices, the cloud's bytes, the origin's bits."""
    if len(want["index"]) == 0:
        assert cloud is None and len(index) == 0
        return
    assert cloud is not None
    assert np.array_equal(index, want["index"])
    got = cloud.download()
    assert got.shape == want["xyz"].shape
    assert got.tobytes() == want["xyz"].tobytes(), int(np.sum(np.any(got.view(np.uint32) != want["xyz"].view(np.uint32), axis=1)))
    assert np.asarray(origin, dtype=f32).tobytes() == want["origin"].tobytes()
