"""GPU tests of the pose graph solve's further terms (include/dliom.h dliom_pose_graph_terms: fixed-frame pose constraints
and the Huber loss) against the CPU model (tests/cpp/pose_graph_model.cc).  The bars are those of
tests/test_gpu_pose_graph.py: `evaluate` 1e-9 relative; `step` within 10 x the difference between the model's own two
linear solvers on the same case; `solve` with equal termination, iteration counts and accept / reject sequences and poses
within 1e-6 m and 1e-6 rad, the fixed frames' included."""
import bisect
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
import pose_graph_terms_common as tc  # noqa: E402
from pose_graph_common import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    import __graft_entry__
    d = __graft_entry__.build()
    if d.device_count() <= 0:
        pytest.fail("no HIP device")
    return d


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph_model")
    return pc.build_model(d), d


def relative(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("huber_scale", [0.0, tc.EVALUATE_HUBER_SCALE])
@pytest.mark.parametrize("fix_z", [False, True])
def test_evaluate(dl, ctx, model, fix_z, huber_scale):
    """Two fixed frames, one on the frozen submap's nodes; under fix_z a fixed frame keeps its z column (mask 15)."""
    exe, d = model
    g = tc.evaluate_graph(fix_z, huber_scale)
    assert len(g.submaps) <= 8 and len(g.nodes) == 200 and len(g.frames) == 2
    cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
    got_cost, got_residuals, got_gradient = g.device(dl, ctx).evaluate()
    print("cost", abs(got_cost - cost) / cost, "residuals", relative(got_residuals, residuals), "gradient", relative(got_gradient, gradient))
    assert abs(got_cost - cost) <= 1e-9 * cost
    assert relative(got_residuals, residuals) <= 1e-9 and relative(got_gradient, gradient) <= 1e-9
    assert np.array_equal(got_gradient == 0, gradient == 0)  # the same slots are outside the problem
    frames = got_gradient[len(g.submaps) + len(g.nodes):]
    assert np.all(frames[:, :4] != 0) and np.all(frames[:, 4:] == 0)  # z stays a column under fix_z


BOUNDARY = {"s42_f2": (42, 2, False, 256), "s42_f3": (42, 3, False, 260), "s51_f1_fix_z": (51, 1, True, 256),
            "s51_f2_fix_z": (51, 2, True, 260)}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_step_at_the_one_workgroup_boundary(dl, ctx, model, name):
    """Reduced dimensions 256 (one workgroup) and 260 (blocked), reached through the fixed frames' columns."""
    exe, d = model
    submaps, frames, fix_z, dimension = BOUNDARY[name]
    g = tc.boundary_graph(submaps, frames, fix_z)
    qr, eliminated = pc.model_step(exe, g, d, pc.SPARSE_QR), pc.model_step(exe, g, d, pc.ELIMINATED)
    cpu = relative(eliminated["delta"], qr["delta"])
    delta, change, got_dimension = g.device(dl, ctx).step(1e4)
    got = relative(delta, qr["delta"])
    print(name, "reduced dimension", got_dimension, "cpu solvers differ by", cpu, "device from QR", got, "model cost change",
          abs(change - qr["model_cost_change"]) / qr["model_cost_change"])
    assert got_dimension == dimension == qr["columns"] - (5 if fix_z else 6) * len(g.nodes)
    assert cpu > 0
    assert got <= 10 * cpu
    assert abs(change - qr["model_cost_change"]) <= 1e-9 * qr["model_cost_change"]
    assert np.array_equal(delta == 0, qr["delta"] == 0)


def solve_both(dl, ctx, exe, d, g):
    p = g.device(dl, ctx)
    return pc.model_solve(exe, g, d), p, p.solve()


def assert_equal_solves(name, g, want, p, summary):
    got = np.concatenate([p.submaps, p.nodes, p.fixed_frames])
    model_poses = np.concatenate([want["submaps"], want["nodes"], want["frames"]])
    dt = np.linalg.norm(got[:, :3] - model_poses[:, :3], axis=1).max()
    dq = pc.rotation_angles(got, model_poses).max()
    print(name, summary["termination_type"], summary["num_iterations"], summary["steps"], "dt", dt, "dq", dq, "cost",
          summary["final_cost"], want["final_cost"])
    assert summary["termination_type"] == want["termination"]
    assert (summary["num_iterations"], summary["num_successful_steps"], summary["num_unsuccessful_steps"]) == (
        want["iterations"], want["successful"], want["unsuccessful"])
    assert summary["steps"] == want["steps"]
    assert dt <= 1e-6 and dq <= 1e-6
    assert abs(summary["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    assert abs(summary["initial_cost"] - want["initial_cost"]) <= 1e-9 * want["initial_cost"]
    assert summary["linear_solver_failures"] == 0


@pytest.fixture(scope="module")
def solved(dl, ctx, model):
    """Every case of the list solved once by the model and once on the device."""
    exe, d = model
    out = {}

    def get(name):
        if name not in out:
            g = tc.CASES[name](exe, d)
            out[name] = (g,) + solve_both(dl, ctx, exe, d, g)
        return out[name]
    return get


@pytest.mark.parametrize("name", list(tc.CASES))
def test_solve(solved, name):
    g, want, p, summary = solved(name)
    assert_equal_solves(name, g, want, p, summary)
    assert summary["reduced_dimension"] == want["columns"] - 6 * int((g.node_constant == 0).sum())
    if len(g.frames):
        assert p.fixed_frames.tobytes() != g.frames.tobytes()
        assert np.all(p.fixed_frames[:, 4:6] == 0)  # a yaw-only start stays yaw-only


def test_the_loss_does_its_job(dl, ctx, model):
    """12 submaps x 20 nodes on a known truth with one inter-submap constraint 5 m wrong: the nodes end nearer the truth
    under HuberLoss than under TrivialLoss -- on the model, and the device equals the model in both runs."""
    exe, d = model
    errors = {}
    for scale in (0.0, tc.LOSS_HUBER_SCALE):
        g, truth = tc.loss_pair(scale)
        assert len(g.submaps) == 12 and len(g.nodes) == 240
        want, p, summary = solve_both(dl, ctx, exe, d, g)
        assert_equal_solves("huber_scale %g" % scale, g, want, p, summary)
        errors[scale] = (tc.node_error(truth, want["nodes"]), tc.node_error(truth, p.nodes))
    print("node error, model and device:", errors)
    assert errors[tc.LOSS_HUBER_SCALE][0] < errors[0.0][0]
    assert errors[tc.LOSS_HUBER_SCALE][1] < errors[0.0][1]


@pytest.mark.parametrize("name", ["s6_n120_loss_and_frames", "s12_n240_frame_rejects_30"])
def test_two_solves_with_terms_are_bit_identical(dl, ctx, solved, name):
    g, _, p, summary = solved(name)
    again = g.device(dl, ctx)
    stats = ctx.memory_stats()
    summary2 = again.solve()
    assert ctx.memory_stats() == stats
    assert again.submaps.tobytes() == p.submaps.tobytes() and again.nodes.tobytes() == p.nodes.tobytes()
    assert again.fixed_frames.tobytes() == p.fixed_frames.tobytes()
    assert (summary2["final_cost"], summary2["initial_cost"], summary2["steps"]) == (summary["final_cost"], summary["initial_cost"], summary["steps"])


@pytest.mark.parametrize("name", ["reduces_noise", "s44_n900_nonmonotonic_50"])
def test_entry_points_are_bit_identical(dl, ctx, model, name):
    """The old entry point, the new one with NULL and the new one with an empty struct (s44: 260 columns, the blocked
    factorisation)."""
    exe, d = model
    g = tc.Graph(pc.CASES[name](exe, d))
    results = []
    for entry in ("plain", "null", "terms"):
        p = g.device(dl, ctx, entry=entry)
        assert p.entry == entry
        cost, residuals, gradient = p.evaluate()
        delta, change, dimension = p.step(1e4)
        summary = p.solve()
        results.append((cost, residuals.tobytes(), gradient.tobytes(), delta.tobytes(), change, dimension, p.submaps.tobytes(),
                        p.nodes.tobytes(), summary["initial_cost"], summary["final_cost"], summary["steps"],
                        summary["num_iterations"], summary["termination_type"]))
    assert results[0][5] > 256 or name == "reduces_noise"
    assert results[0] == results[1] == results[2]


def test_refusals(dl, ctx):
    """Each refused before anything is launched: no read-back, the memory statistics unchanged, the poses untouched."""
    L = dl.load_library()
    n = dl.C.c_int64()
    L.dliom_ctx_read_backs(ctx.h, dl.C.byref(n))
    read_backs = n.value
    stats = ctx.memory_stats()
    base, truth, inter = tc.synthetic(3, 12, 1, seed=1)
    good = tc.with_fixed_frames(base, truth, [dict(origin=tc._yaw_pose([1.0, 0.0, 0.0], 0.3), nodes=list(range(12)))], seed=1)

    def refused(graph, status, patch=None):
        p = graph.device(dl, ctx, entry="terms")
        if patch is not None:
            patch(p)
        before = (p.submaps.copy(), p.nodes.copy(), p.fixed_frames.copy())
        for call in (p.solve, p.evaluate, p.step):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == status
        for a, b in zip(before, (p.submaps, p.nodes, p.fixed_frames)):
            assert np.array_equal(a, b, equal_nan=True)

    def edited(**arrays):
        g = tc.Graph(good, good.frames.copy(), good.frame_constraints.copy(), good.huber_scale, good.inter_submap)
        for key, (index, value) in arrays.items():
            getattr(g, key.split("__")[0])[key.split("__")[1]][index] = value
        return g
    refused(edited(frame_constraints__submap=(2, 1)), dl.ERR_INVALID_ARGUMENT)    # a fixed-frame index out of range
    refused(edited(frame_constraints__submap=(2, -1)), dl.ERR_INVALID_ARGUMENT)
    refused(edited(frame_constraints__node=(2, 12)), dl.ERR_INVALID_ARGUMENT)     # a node index out of range
    for scale in (-1.0, np.nan, np.inf):
        refused(tc.Graph(good, good.frames, good.frame_constraints, scale, inter), dl.ERR_INVALID_ARGUMENT)

    # a positive count with a NULL array: the binding cannot say that, so the struct is patched
    class Patched(dl.PoseGraph):
        def _call(self, name, *rest):
            terms = dl.PoseGraphTerms(self.counts[0], self.pointers[0], self.counts[1], self.pointers[1], 0.0, None)
            dl._check(getattr(self._L, "dliom_pose_graph_%s_terms" % name)(self.ctx.h, dl.C.byref(self.options), *self._graph(),
                                                                           dl.C.byref(terms), *rest), name)
    for counts, keep in (((1, 0), None), ((1, len(good.frame_constraints)), 0), ((-1, 0), None), ((0, -1), None)):
        p = Patched(ctx, good.submaps, good.nodes, good.constraints, fixed_frame_poses=good.frames,
                    fixed_frame_constraints=good.frame_constraints)
        p.counts = counts
        p.pointers = [None, None]
        if keep is not None:
            p.pointers[keep] = dl._p(p.fixed_frames, dl._f64p)
        for call in (p.solve, p.evaluate, p.step):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == dl.ERR_INVALID_ARGUMENT
    nan = edited()
    nan.frames[0, 5] = np.nan
    refused(nan, dl.ERR_SOLVER)
    nan = edited()
    nan.frame_constraints["zbar"][3, 2] = np.inf
    refused(nan, dl.ERR_SOLVER)
    nan = edited()
    nan.frame_constraints["rotation_weight"][1] = np.nan
    refused(nan, dl.ERR_SOLVER)
    # 1 365 free submaps: 2 + 6 * 1 364 = 8 186 columns, under the cap of 8 192 without the two fixed frames' 8
    big, big_truth, _ = tc.synthetic(1365, 1364, 0, seed=2)
    two = [dict(origin=tc._yaw_pose([0.0, 0.0, 0.0], 0.1 * f), nodes=[f, f + 2]) for f in range(2)]
    refused(tc.with_fixed_frames(big, big_truth, two, seed=2), dl.ERR_TOO_LARGE)
    L.dliom_ctx_read_backs(ctx.h, dl.C.byref(n))
    assert n.value == read_backs and ctx.memory_stats() == stats
    assert good.device(dl, ctx).step(1e4)[2] == 2 + 6 * 2 + 4  # the unedited graph is accepted


# ---- the adapter: optimization_problem_3d.cc:78-102 and :491-548 restated with Python floats, operation for operation -------
def _rotate(q, v):
    w, x, y, z = (float(c) for c in q)
    uv = [2. * (y * v[2] - z * v[1]), 2. * (z * v[0] - x * v[2]), 2. * (x * v[1] - y * v[0])]
    return [v[0] + w * uv[0] + (y * uv[2] - z * uv[1]), v[1] + w * uv[1] + (z * uv[0] - x * uv[2]), v[2] + w * uv[2] + (x * uv[1] - y * uv[0])]


def _inverse(a):
    q = [float(a[3]), -float(a[4]), -float(a[5]), -float(a[6])]
    t = _rotate(q, [float(c) for c in a[:3]])
    return [-t[0], -t[1], -t[2]] + q


def _multiply(a, b):
    t = _rotate(a[3:], [float(c) for c in b[:3]])
    pw, px, py, pz = (float(c) for c in a[3:])
    qw, qx, qy, qz = (float(c) for c in b[3:])
    w = pw * qw - px * qx - py * qy - pz * qz
    x = pw * qx + px * qw + py * qz - pz * qy
    y = pw * qy + py * qw + pz * qx - px * qz
    z = pw * qz + pz * qw + px * qy - py * qx
    norm = math.sqrt(w * w + x * x + y * y + z * z)
    return [t[0] + float(a[0]), t[1] + float(a[1]), t[2] + float(a[2]), w / norm, x / norm, y / norm, z / norm]


def _yaw_only(a):
    direction = _rotate(a[3:], [1., 0., 0.])
    yaw = math.atan2(direction[1], direction[0])
    return [float(a[0]), float(a[1]), float(a[2]), math.cos(yaw / 2.), 0., 0., math.sin(yaw / 2.)]


def _interpolate_transforms(start_time, start, end_time, end, time):
    duration = float(end_time - start_time) / 1e7
    factor = float(time - start_time) / 1e7 / duration
    origin = [float(start[k]) + (float(end[k]) - float(start[k])) * factor for k in range(3)]
    p, q = [float(c) for c in start[3:]], [float(c) for c in end[3:]]
    d = p[0] * q[0] + p[1] * q[1] + p[2] * q[2] + p[3] * q[3]
    scale0, scale1 = 1. - factor, factor
    if not abs(d) >= 1. - 2.220446049250313e-16:
        theta = math.acos(abs(d))
        sin_theta = math.sin(theta)
        scale0 = math.sin((1. - factor) * theta) / sin_theta
        scale1 = math.sin(factor * theta) / sin_theta
    if d < 0.:
        scale1 = -scale1
    return origin + [scale0 * p[k] + scale1 * q[k] for k in range(4)]


def _interpolate(samples, time):
    """samples: [(time, pose or None)] by time -> the pose at `time` or None (Interpolate, :78-102)"""
    at = bisect.bisect_left([t for t, _ in samples], time)
    if at == len(samples) or samples[at][1] is None:
        return None
    if at == 0:
        return [float(c) for c in samples[0][1]] if samples[0][0] == time else None
    if samples[at - 1][1] is None:
        return None
    return _interpolate_transforms(samples[at - 1][0], samples[at - 1][1], samples[at][0], samples[at][1], time)


def test_adapter(dl, ctx, tmp_path):
    """tests/cpp/pose_graph_terms_adapter.cc -- two trajectories through AddFixedFramePoseData and Solve, one with a gap in
    its fixed-frame data, one with a sample exactly at its first node's time, tagged constraints and a huber_scale --
    against the Python binding fed by the restatement above, bit for bit; the second Solve starts from the stored origin.
    Like tests/test_gpu_pose_graph.py::test_adapter a SELF-COMPARISON of two routes into one entry point: it checks the
    adapter's host steps, not the solve."""
    exe = str(tmp_path / "pose_graph_terms_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "pose_graph_terms_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    g, truth, inter = tc.synthetic(7, 41, 1, seed=9, nonmonotonic=True, max_iterations=12)
    S, N = len(g.submaps), len(g.nodes)
    huber_scale = tc.LOSS_HUBER_SCALE
    node_time = lambda j: 1000 + j * 10000000  # noqa: E731
    rng = np.random.RandomState(9)
    origins = [tc._yaw_pose([1.0, 2.0, 0.0], 0.4), tc._yaw_pose([-2.0, 0.5, 0.3], -1.0)]

    def sample(trajectory, time):
        j = min(max(int(round((time - 1000) / 1e7)), 0), N - 1)
        z = synth.pose7_compose(synth.pose7_inverse(origins[trajectory]), truth[j])
        return synth.pose7_compose(z, np.concatenate([rng.normal(0, 0.05, 3), synth._quat_of(rng.normal(0, 0.01, 3))]))
    # trajectory 0: samples off the nodes' times, the fourth without a pose (a gap); trajectory 1: the first sample exactly
    # at its first node's time, and data that ends before the trajectory does
    times = [[1000 - 5000000 + k * 25000000 for k in range(18)], [node_time(1) + k * 30000000 for k in range(10)]]
    samples = [[(t, None if (trajectory, k) == (0, 3) else sample(trajectory, t)) for k, t in enumerate(times[trajectory])]
               for trajectory in range(2)]
    src, dst = str(tmp_path / "graph.bin"), str(tmp_path / "adapter.bin")
    pc.write_adapter_graph(g, src)
    with open(src, "ab") as f:
        f.write(inter.astype("<i4").tobytes() + struct.pack("<d", huber_scale))
        for trajectory in range(2):
            f.write(struct.pack("<i", len(samples[trajectory])))
            for t, pose in samples[trajectory]:
                f.write(struct.pack("<qi7d", t, pose is not None, *(np.zeros(7) if pose is None else pose)))
    subprocess.check_call([exe, src, dst])
    data = open(dst, "rb").read()
    record = np.dtype([("poses", "<f8", (S + N, 7)), ("origins", [("has", "<i4"), ("pose", "<f8", 7)], 2), ("termination", "<i4"),
                       ("iterations", "<i4"), ("final_cost", "<f8")])
    assert len(data) == 2 * record.itemsize
    adapter = np.frombuffer(data, dtype=record)
    # the same graph in the adapter's MapById order: trajectory 0 (even inputs), then trajectory 1 (odd inputs)
    submap_order = np.r_[np.arange(0, S, 2), np.arange(1, S, 2)]
    node_order = np.r_[np.arange(0, N, 2), np.arange(1, N, 2)]
    constraints = g.constraints.copy()
    constraints["submap"] = np.argsort(submap_order)[g.constraints["submap"]]
    constraints["node"] = np.argsort(node_order)[g.constraints["node"]]
    submaps, nodes, stored = g.submaps[submap_order], g.nodes[node_order], [None, None]
    for solve in range(2):
        frames, rows, interpolated = [], [], [0, 0]
        for trajectory in range(2):
            first = True
            for index, j in enumerate(node_order):
                if j % 2 != trajectory:
                    continue
                z = _interpolate(samples[trajectory], node_time(j))
                if z is None:
                    continue
                interpolated[trajectory] += 1
                if first:
                    frames.append(_yaw_only(stored[trajectory] if stored[trajectory] is not None else _multiply(nodes[index], _inverse(z))))
                    first = False
                rows.append((len(frames) - 1, index, z, 2e1, 3e2))
        frame_constraints = np.zeros(len(rows), dtype=pc.CONSTRAINT)
        for i, row in enumerate(rows):
            frame_constraints[i] = row
        if solve == 0:  # the gap and the early end leave nodes without a fixed-frame constraint; the exact hit counts
            assert (N, interpolated) == (41, [21 - 2, 14])  # nodes 6 and 8 fall into the gap; the data ends behind node 27
            assert rows[interpolated[0]][1] == np.argsort(node_order)[1]
            assert np.array_equal(rows[interpolated[0]][2], samples[1][0][1])
        p = dl.PoseGraph(ctx, submaps, nodes, constraints, None, None, 0, g.fix_z, g.nonmonotonic, g.max_iterations,
                         fixed_frame_poses=np.array(frames), fixed_frame_constraints=frame_constraints, huber_scale=huber_scale,
                         inter_submap=inter)
        summary = p.solve()
        got = adapter[solve]
        assert (summary["termination_type"], summary["num_iterations"], summary["final_cost"]) == (
            got["termination"], got["iterations"], got["final_cost"])
        assert got["poses"][:S][submap_order].tobytes() == p.submaps.tobytes() and got["poses"][S:][node_order].tobytes() == p.nodes.tobytes()
        assert list(got["origins"]["has"]) == [1, 1] and got["origins"]["pose"].tobytes() == p.fixed_frames.tobytes()
        print("solve", solve, summary["termination_type"], summary["num_iterations"], summary["steps"], summary["final_cost"])
        if solve == 0:  # the second starts where the first ended and may have nothing left to do
            assert summary["num_successful_steps"] >= 2 and p.fixed_frames.tobytes() != np.array(frames).tobytes()
        submaps, nodes, stored = p.submaps, p.nodes, [p.fixed_frames[0], p.fixed_frames[1]]
    assert adapter[0]["poses"].tobytes() != adapter[1]["poses"].tobytes() or adapter[1]["iterations"] == 1
