"""LocalTrajectoryBuilder3D's initialisation modes (d-liom_amd/cpp/dliom_cartographer.h) fed from the first message:
tests/cpp/ltb3d_init_adapter.cc streams 200 Hz IMU and 10 small scans through the adapter.  In NDT mode the state handed to
InitializeIMU equals, TO THE LAST BIT, the same chain composed here from the ctypes calls (ImuIntegrator, NdtScanMatcher,
imu_lidar_align_with_world -- the library's own solver, not the numpy model -- with the guess and the frames in the float
and double arithmetic the adapter states)."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imu_lidar_init_common as il  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = [0.08, 0.004, 4e-5, 2e-6]
G = 9.80511
T, SCANS, IMU_PER_SCAN = 0.1, 10, 20
F_DYNAMIC, F_STATIC = 7, 2
DEFAULT, STATIC, NDT = 0, 1, 2
f32 = np.float32


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    libdir = os.path.join(ROOT, "d-liom_amd")
    out = str(tmp_path_factory.mktemp("ltb3d_init") / "ltb3d_init_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(libdir, "cpp"), "-o", out, os.path.join(ROOT, "tests", "cpp", "ltb3d_init_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    return out


@pytest.fixture(scope="module")
def scans():
    """Ten 16 x 128 scans of the room with point times, from a sensor that creeps (2 cm radius): [x, y, z, t] rows.  The
    room is scaled to a quarter, as in tests/test_gpu_ndt_scan_matcher.py: at its own size 2048 points leave NDT two valid
    cells, scaled about 75"""
    from dliom import synth
    synth.set_trajectory(0.02, 4.0, 0.02)
    try:
        out = [np.ascontiguousarray(synth.moving_scan(T * k, 16, 128), np.float32) for k in range(1, SCANS + 1)]
    finally:
        synth.set_trajectory()
    for s in out:
        s[:, :3] *= f32(0.25)
    assert len({len(s) for s in out}) == 1
    return out


def imu_rows(excited):
    """(SCANS, IMU_PER_SCAN, 7) rows dt, acc, gyr at 200 Hz.  excited: a horizontal acceleration of 1 m/s^2 that swings at
    1.5 and 1.1 Hz over gravity, no rotation -- what AlignWithWorld's gates accept beside frames that barely move; else the
    platform at rest"""
    rows = np.zeros((SCANS, IMU_PER_SCAN, 7))
    for s in range(SCANS):
        for k in range(IMU_PER_SCAN):
            t = T * s + (k + 1) * T / IMU_PER_SCAN
            a = [math.sin(2 * math.pi * 1.5 * t), math.cos(2 * math.pi * 1.1 * t), G] if excited else [0.0, 0.0, G]
            rows[s, k] = [T / IMU_PER_SCAN] + a + [0.0, 0.0, 0.0]
    return rows


def run(dl, exe, tmp_path, scans, rows, mode, set_state_after=-1):
    from test_gpu_parity import FRONT_END_OPTS
    path = str(tmp_path / "stream.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("8i", SCANS, len(scans[0]), IMU_PER_SCAN, mode, F_DYNAMIC, F_STATIC, set_state_after, 0))
        f.write(bytes(dl.front_end_options_struct(FRONT_END_OPTS)))
        f.write(np.asarray(NOISE + [G], np.float64).tobytes())
        for r, s in zip(rows, scans):
            f.write(np.ascontiguousarray(r, np.float64).tobytes())
            f.write(s.tobytes())
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert out.returncode == 0 and "LTB3D INIT ADAPTER DONE" in out.stdout, out.stdout + out.stderr
    per_scan = [dict(zip(ln.split()[2::2], (int(v) for v in ln.split()[3::2]))) for ln in out.stdout.splitlines() if ln.startswith("SCAN")]
    state = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("STATE")]
    assert len(per_scan) == SCANS and len(state) <= 1
    return per_scan, (int(state[0][1]), np.array([float(v) for v in state[0][2:]])) if state else None


def quaternion_of_matrix(m):
    """Eigen's Quaterniond(Matrix3d), as the adapter writes it"""
    m = [float(v) for v in np.asarray(m).reshape(9)]
    q = [1.0, 0.0, 0.0, 0.0]
    t = (m[0] + m[4]) + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[3 * k + j] - m[3 * j + k]) * t
        q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def compose_ndt_mode(dl, ctx, scans, rows):
    """InitilizeByNDT from the ctypes calls -> per scan (frames held, failures), and (scan, state16) of the initialisation"""
    integrator = dl.ImuIntegrator(np.zeros(3), np.zeros(3), NOISE)
    matcher = dl.NdtScanMatcher(ctx)
    frames, velocity, failures, book, state = [], np.zeros(3, f32), 0, [], None
    ticks, last_imu, last_scan = 0, -1, 0
    try:
        for s in range(SCANS):
            for row in rows[s]:
                ticks += int(row[0] * 1e7 + 0.5)
                if state is None:
                    dt = 1.0 / 500.0 if last_imu < 0 else float(ticks - last_imu) * 1e-7
                    last_imu = ticks
                    integrator.push_back(dt, row[1:4], row[4:7])
            if state is not None:
                book.append((len(frames), failures))
                continue
            xyz = np.ascontiguousarray(scans[s][:, :3])
            if not frames:
                assert matcher.match(xyz) is None
                last_scan = ticks
                frames.append((np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), None))
                integrator.reset(np.zeros(3), np.zeros(3))
                book.append((1, failures))
                continue
            dt = f32(float(ticks - last_scan) * 1e-7)
            pre = integrator.get()
            w, x, y, z = (f32(v) for v in pre["delta_q"])
            two = f32(2)
            tx, ty, tz = two * x, two * y, two * z
            twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
            one = f32(1)
            guess = np.array([[one - (tyy + tzz), txy - twz, txz + twy, velocity[0] * dt],
                              [txy + twz, one - (txx + tzz), tyz - twx, velocity[1] * dt],
                              [txz - twy, tyz + twx, one - (txx + tyy), velocity[2] * dt], [0, 0, 0, 1]], f32)
            result = matcher.match(xyz, guess.astype(np.float64))
            transform = result["transform"].astype(f32)
            R, t = transform[:3, :3].astype(np.float64), transform[:3, 3]
            Rp = il.rotation_of(frames[-1][0][3:])
            Rf = [[(float(Rp[r, 0]) * float(R[0, c]) + float(Rp[r, 1]) * float(R[1, c])) + float(Rp[r, 2]) * float(R[2, c]) for c in range(3)]
                  for r in range(3)]
            pose = np.array([float(t[0]), float(t[1]), float(t[2])] + quaternion_of_matrix(Rf))
            frames.append((pose, dict(sum_dt=pre["sum_dt"], delta_p=pre["delta_p"], delta_v=pre["delta_v"])))
            velocity = np.array([t[0] / dt, t[1] / dt, t[2] / dt], f32)
            print("pair", s, "t", t, "iterations", result["iterations"], "pairs", result["pairs"], "reason", result["reason"])
            integrator.reset(np.zeros(3), np.zeros(3))
            last_scan = ticks
            if len(frames) == F_DYNAMIC + 1:
                aligned = dl.imu_lidar_align_with_world(frames, [0, 0, 0, 1, 0, 0, 0], G)
                print("AlignWithWorld outcome", aligned["outcome"], "excitation", aligned["excitation"], "g", aligned["gravity_in_laser"])
                if aligned["outcome"] != dl.INIT_OK:
                    failures += 1
                    frames = frames[:1]
                else:
                    state = (s, np.concatenate([aligned["P"][-1], quaternion_of_matrix(aligned["R"][-1]), aligned["V"][-1], np.zeros(6)]),
                             aligned)
            book.append((len(frames), failures))
    finally:
        matcher.close()
        integrator.close()
    return book, state


def test_ndt_mode_equals_the_composition_and_then_matches(dl, ctx, exe, tmp_path, scans):
    rows = imu_rows(excited=True)
    per_scan, got = run(dl, exe, tmp_path, scans, rows, NDT)
    book, want = compose_ndt_mode(dl, ctx, scans, rows)
    assert want is not None and got is not None, (per_scan, book)
    assert want[0] == got[0] == F_DYNAMIC  # the scan that fills frame F
    print("excitation", want[2]["excitation"], "gravity in laser", want[2]["gravity_in_laser"], "state", got[1][:10])
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])  # P, R, V to the last bit
    assert not got[1][10:].any()  # the biases are zero
    assert [(p["frames"], p["failures"]) for p in per_scan] == book
    # nothing is returned until initialised, the scan that initialises included; the scan after it returns a MatchingResult
    assert [p["result"] for p in per_scan] == [0] * (F_DYNAMIC + 1) + [1] * (SCANS - F_DYNAMIC - 1)
    assert [p["initialised"] for p in per_scan] == [0] * F_DYNAMIC + [1] * (SCANS - F_DYNAMIC)
    assert abs(np.linalg.norm(want[2]["gravity_in_laser"]) - G) < 0.2


def test_ndt_mode_at_rest_starts_over(dl, ctx, exe, tmp_path, scans):
    """No excitation: AlignWithWorld fails at F + 1 frames, the frame count goes back to 1 and nothing is returned"""
    rows = imu_rows(excited=False)
    per_scan, got = run(dl, exe, tmp_path, scans, rows, NDT)
    book, want = compose_ndt_mode(dl, ctx, scans, rows)
    assert got is None and want is None
    assert [(p["frames"], p["failures"]) for p in per_scan] == book
    assert [p["frames"] for p in per_scan] == [1, 2, 3, 4, 5, 6, 7, 1, 2, 3] and per_scan[-1]["failures"] == 1
    assert not any(p["result"] or p["initialised"] for p in per_scan)


def test_static_mode(dl, exe, tmp_path, scans):
    """The scan after frames_for_static_initialization + 1 earlier ones initialises from every IMU sample buffered so far"""
    rows = imu_rows(excited=False)
    rows[:, :, 1:4] += np.array([0.4, -0.3, 0.05])  # a tilted, biased accelerometer
    rows[:, :, 4:7] += np.array([1e-3, -2e-3, 5e-4])
    per_scan, got = run(dl, exe, tmp_path, scans, rows, STATIC)
    at = F_STATIC + 1
    assert got is not None and got[0] == at
    buffered = rows[:at + 1].reshape(-1, 7)
    want = dl.imu_static_initialization(buffered[:, 1:4], buffered[:, 4:7], G)
    state = np.concatenate([want["P"], quaternion_of_matrix(want["R"]), want["V"], want["ba"], want["bg"]])
    assert got[1].tobytes() == state.tobytes(), (got[1], state)
    assert [p["result"] for p in per_scan] == [0] * (at + 1) + [1] * (SCANS - at - 1)
    assert [p["initialised"] for p in per_scan] == [0] * at + [1] * (SCANS - at)


@pytest.mark.parametrize("set_state_after", [-1, 4])
def test_default_mode_still_drops_everything_before_set_initial_state(dl, exe, tmp_path, scans, set_state_after):
    per_scan, got = run(dl, exe, tmp_path, scans, imu_rows(excited=True), DEFAULT, set_state_after)
    first = SCANS if set_state_after < 0 else set_state_after + 1
    assert [p["result"] for p in per_scan] == [0] * first + [1] * (SCANS - first)
    assert all(p["frames"] == 0 and p["failures"] == 0 for p in per_scan)
    assert (got is None) == (set_state_after < 0)
