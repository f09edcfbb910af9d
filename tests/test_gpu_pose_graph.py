"""GPU tests of the pose graph solve (include/dliom.h "pose graph optimisation", d-liom_amd/csrc/pose_graph.hip) against
the CPU model (tests/cpp/pose_graph_model.cc).  Bars: poses after a solve within 1e-6 m and 1e-6 rad (the angle of
the relative rotation, pose by pose) with equal iteration counts and accept / reject sequences (the bar of CeresScanMatcher3D,
tests/test_gpu_full_size.py); `evaluate` against the model's Jets 1e-9 relative (tests/test_gpu_parity.py); `step`
against the model's QR step within 10 x the difference between the model's own two linear solvers, measured on the CPU
for the same case when the test runs (DESIGN 3.15 lists the values)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402

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


@pytest.mark.parametrize("fix_z", [False, True])
def test_evaluate(dl, ctx, model, fix_z):
    exe, d = model
    g = pc.branches_graph(fix_z)
    cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
    got_cost, got_residuals, got_gradient = g.device(dl, ctx).evaluate()
    print("cost", abs(got_cost - cost) / cost, "residuals", relative(got_residuals, residuals), "gradient", relative(got_gradient, gradient))
    assert abs(got_cost - cost) <= 1e-9 * cost
    assert relative(got_residuals, residuals) <= 1e-9 and relative(got_gradient, gradient) <= 1e-9
    assert np.array_equal(got_gradient == 0, gradient == 0)  # the same slots are outside the problem


def step_cases():
    """name -> graph: every branch; the 1e-9 weights (the LM clamp is the whole diagonal of submap 2); reduced dimensions
    2 + 6 (S - 1) (5 under fix_z) on either side of one panel (32) and of the one-workgroup limit (256)."""
    yield "branches", lambda e, d: pc.branches_graph(False)
    yield "branches_fix_z", lambda e, d: pc.branches_graph(True)
    yield "reduces_noise", lambda e, d: pc.reduces_noise(e, d)[0]
    for s, fix_z in ((6, False), (7, False), (43, False), (44, False), (7, True), (8, True), (51, True), (52, True)):
        yield "s%d%s" % (s, "_fix_z" if fix_z else ""), (lambda e, d, s=s, f=fix_z: pc.synthetic(s, 2 * (s - 1), 1, seed=s, fix_z=f))


STEP_DIMENSIONS = {"s6": 32, "s7": 38, "s43": 254, "s44": 260, "s7_fix_z": 32, "s8_fix_z": 37, "s51_fix_z": 252, "s52_fix_z": 257,
                   "reduces_noise": 14}


@pytest.mark.parametrize("name,make", list(step_cases()))
def test_step(dl, ctx, model, name, make):
    exe, d = model
    g = make(exe, d)
    qr, eliminated = pc.model_step(exe, g, d, pc.QR), pc.model_step(exe, g, d, pc.ELIMINATED)
    cpu = relative(eliminated["delta"], qr["delta"])
    delta, change, dimension = g.device(dl, ctx).step(1e4)
    got = relative(delta, qr["delta"])
    print(name, "reduced dimension", dimension, "cpu solvers differ by", cpu, "device from QR", got, "model cost change",
          abs(change - qr["model_cost_change"]) / qr["model_cost_change"])
    assert name not in STEP_DIMENSIONS or dimension == STEP_DIMENSIONS[name]
    assert cpu > 0
    assert got <= 10 * cpu
    assert abs(change - qr["model_cost_change"]) <= 1e-9 * qr["model_cost_change"]
    assert np.array_equal(delta == 0, qr["delta"] == 0)


def test_step_above_65535_constraints(dl, ctx, model):
    """350 submaps x 100 nodes (70 000 constraints and more, reduced dimension 2 096: 66 panels of the chip-wide
    factorisation, the one-workgroup triangular solves on a large system).  The device step's normal-equation residual
    ||(H + D^2) y + g|| / ||g||, formed in numpy from the MODEL's sparse Jacobian on the scaled columns, against 10 x the
    residual of scipy.sparse.linalg.spsolve on the same system."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    exe, d = model
    radius = 1e4
    g = pc.synthetic(350, 35000, 35, seed=350)
    assert len(g.constraints) > 65535
    lin = pc.model_step(exe, g, d, pc.LINEARISE_ONLY, radius)
    delta, change, dimension = g.device(dl, ctx).step(radius)
    assert dimension == 2096 == 2 + 6 * 349
    scale = lin["scale"].reshape(-1)
    active = np.flatnonzero(scale > 0)
    column = np.full(len(scale), -1)
    column[active] = np.arange(len(active))
    blocks = lin["blocks"]
    assert len(blocks) == len(g.constraints) and lin["columns"] == len(active)
    rows = (6 * np.arange(len(blocks))[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), dtype=np.int64)
    parts = []
    for key, pose in (("js", g.constraints["submap"][blocks["c"]]), ("jn", len(g.submaps) + g.constraints["node"][blocks["c"]])):
        slots = 6 * pose[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), dtype=np.int64)
        values = blocks[key] * scale[slots]
        keep = column[slots] >= 0
        parts.append(sp.coo_matrix((values[keep], (rows[keep], column[slots][keep])), shape=(6 * len(blocks), len(active))))
    jacobian = (parts[0] + parts[1]).tocsr()
    r = blocks["r"].reshape(-1)
    hessian = (jacobian.T @ jacobian).tocsc()
    hessian = hessian + sp.diags(np.clip(hessian.diagonal(), 1e-6, 1e32) / radius)
    gradient = jacobian.T @ r
    y = delta.reshape(-1)[active] / scale[active]
    device = np.linalg.norm(hessian @ y + gradient) / np.linalg.norm(gradient)
    # spsolve on the same system with the nodes' columns ordered first and no further column permutation: its fill-in is
    # then the submaps' Schur complement (0.2 s; 20 s in the default ordering)
    order = np.r_[np.arange(dimension, len(active)), np.arange(dimension)]
    solution = np.empty(len(active))
    solution[order] = spsolve(hessian[order][:, order].tocsc(), -gradient[order], permc_spec="NATURAL")
    reference = np.linalg.norm(hessian @ solution + gradient) / np.linalg.norm(gradient)
    model_change = -float((jacobian @ y) @ (r + (jacobian @ y) / 2))
    print("normal-equation residual: device", device, "spsolve", reference, "model cost change", change, model_change)
    assert reference > 0 and device <= 10 * reference
    assert abs(change - model_change) <= 1e-9 * model_change


@pytest.fixture(scope="module")
def solved(dl, ctx, model):
    """Every case of the list solved once by the model and once on the device."""
    exe, d = model
    out = {}

    def get(name):
        if name not in out:
            g = pc.CASES[name](exe, d)
            p = g.device(dl, ctx)
            out[name] = (g, pc.model_solve(exe, g, d), p, p.solve())
        return out[name]
    return get


@pytest.mark.parametrize("name", list(pc.CASES))
def test_solve(solved, name):
    g, want, p, summary = solved(name)
    got, model_poses = np.concatenate([p.submaps, p.nodes]), np.concatenate([want["submaps"], want["nodes"]])
    dt = np.linalg.norm(got[:, :3] - model_poses[:, :3], axis=1).max()
    dq = pc.rotation_angles(got, model_poses).max()
    print(name, summary["termination_type"], summary["num_iterations"], summary["steps"], "dt", dt, "dq", dq, "cost",
          summary["final_cost"], want["final_cost"])
    assert summary["termination_type"] == want["termination"]
    assert (summary["num_iterations"], summary["num_successful_steps"], summary["num_unsuccessful_steps"]) == (
        want["iterations"], want["successful"], want["unsuccessful"])
    assert summary["steps"] == want["steps"]
    assert summary["reduced_dimension"] == sum(2 if a == g.gravity else (5 if g.fix_z else 6)
                                               for a in range(len(g.submaps)) if not g.submap_constant[a])
    assert dt <= 1e-6 and dq <= 1e-6
    assert abs(summary["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    assert abs(summary["initial_cost"] - want["initial_cost"]) <= 1e-9 * want["initial_cost"]
    assert summary["linear_solver_failures"] == 0


def test_reduces_noise_on_the_device(solved, model):
    """optimization_problem_3d_test.cc:189-190 on the device's result."""
    exe, d = model
    _, truth = pc.reduces_noise(exe, d)
    g, _, p, _ = solved("reduces_noise")
    before, after = pc.noise_errors(truth, g.nodes), pc.noise_errors(truth, p.nodes)
    print("ratios", after[0] / before[0], after[1] / before[1])
    assert 0.8 * before[0] > after[0] and 0.8 * before[1] > after[1]


@pytest.mark.parametrize("name", ["reduces_noise", "s44_n900_nonmonotonic_50"])
def test_two_solves_are_bit_identical(dl, ctx, solved, name):
    g, _, p, summary = solved(name)
    again = g.device(dl, ctx)
    stats = ctx.memory_stats()
    summary2 = again.solve()
    assert ctx.memory_stats() == stats  # scratch is allocated and released inside the call
    assert again.submaps.tobytes() == p.submaps.tobytes() and again.nodes.tobytes() == p.nodes.tobytes()
    assert (summary2["final_cost"], summary2["steps"]) == (summary["final_cost"], summary["steps"])


def test_constraint_order_does_not_matter(dl, ctx, solved):
    g, _, p, summary = solved("s12_n240_nonmonotonic_50")
    order = np.random.RandomState(3).permutation(len(g.constraints))
    shuffled = pc.Graph(g.submaps, g.nodes, g.constraints[order], g.submap_constant, g.node_constant, g.gravity, g.fix_z,
                        g.nonmonotonic, g.max_iterations).device(dl, ctx)
    summary2 = shuffled.solve()
    assert summary2["steps"] == summary["steps"]
    for a, b in ((shuffled.nodes, p.nodes), (shuffled.submaps, p.submaps)):
        assert np.linalg.norm(a[:, :3] - b[:, :3], axis=1).max() <= 1e-6 and pc.rotation_angles(a, b).max() <= 1e-6


def test_refusals(dl, ctx):
    """Each refused before anything is launched: no read-back, no synchronisation, the poses untouched."""
    def refused(graph, status):
        p = graph.device(dl, ctx)
        before = (p.submaps.copy(), p.nodes.copy())
        for call in (p.solve, p.evaluate, p.step):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == status
        assert np.array_equal(p.submaps, before[0], equal_nan=True) and np.array_equal(p.nodes, before[1], equal_nan=True)
    n = dl.C.c_int64()
    dl.load_library().dliom_ctx_read_backs(ctx.h, dl.C.byref(n))
    read_backs = n.value
    base = pc.synthetic(3, 12, 0, seed=1)
    bad = pc.Graph(base.submaps, base.nodes, base.constraints.copy())
    bad.constraints["submap"][2] = 3
    refused(bad, dl.ERR_INVALID_ARGUMENT)
    bad = pc.Graph(base.submaps, base.nodes, base.constraints.copy())
    bad.constraints["node"][2] = -1
    refused(bad, dl.ERR_INVALID_ARGUMENT)
    refused(pc.Graph(base.submaps, base.nodes, base.constraints, gravity=3), dl.ERR_INVALID_ARGUMENT)
    nan = pc.Graph(base.submaps, base.nodes.copy(), base.constraints)
    nan.nodes[7, 4] = np.nan
    refused(nan, dl.ERR_SOLVER)
    # 1 367 free submaps: 2 + 6 * 1 366 = 8 198 columns, above the cap of 8 192
    big = pc.synthetic(1367, 1366, 0, seed=2)
    refused(big, dl.ERR_TOO_LARGE)
    dl.load_library().dliom_ctx_read_backs(ctx.h, dl.C.byref(n))
    assert n.value == read_backs


@pytest.mark.parametrize("frozen", [None, 1])
def test_adapter(dl, ctx, model, tmp_path, frozen):
    """mapping::optimization::OptimizationProblem3D of dliom_cartographer.h (tests/cpp/pose_graph_adapter.cc: Add / Insert
    / Trim / SetMaxNumIterations / Solve over two trajectories, so that the ids' order is not the input's) against the
    Python binding on the same graph, bit for bit.  This is a SELF-COMPARISON of two routes into one entry point: it
    checks the adapter's compaction of ids, its constant flags and its write-back, not the solve."""
    import subprocess
    exe = str(tmp_path / "pose_graph_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "pose_graph_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    g = pc.synthetic(7, 41, 1, seed=9, fix_z=frozen is not None, nonmonotonic=True, max_iterations=12)
    src, dst = str(tmp_path / "graph.bin"), str(tmp_path / "adapter.bin")
    pc.write_adapter_graph(g, src)
    subprocess.check_call([exe, src, dst] + ([] if frozen is None else [str(frozen)]))
    data = open(dst, "rb").read()
    S, N = len(g.submaps), len(g.nodes)
    poses = np.frombuffer(data, dtype=np.float64, count=7 * (S + N)).reshape(-1, 7)
    termination, iterations = np.frombuffer(data, dtype=np.int32, count=2, offset=56 * (S + N))
    final_cost = np.frombuffer(data, dtype=np.float64, count=1, offset=56 * (S + N) + 8)[0]
    # the same graph in the adapter's MapById order: trajectory 0 (even inputs), then trajectory 1 (odd inputs)
    submap_order = np.r_[np.arange(0, S, 2), np.arange(1, S, 2)]
    node_order = np.r_[np.arange(0, N, 2), np.arange(1, N, 2)]
    constraints = g.constraints.copy()
    constraints["submap"] = np.argsort(submap_order)[g.constraints["submap"]]
    constraints["node"] = np.argsort(node_order)[g.constraints["node"]]
    p = pc.Graph(g.submaps[submap_order], g.nodes[node_order], constraints,
                 (submap_order % 2 == 1).astype(np.uint8) if frozen == 1 else None,
                 (node_order % 2 == 1).astype(np.uint8) if frozen == 1 else None, 0, g.fix_z, g.nonmonotonic,
                 g.max_iterations).device(dl, ctx)
    summary = p.solve()
    assert (summary["termination_type"], summary["num_iterations"], summary["final_cost"]) == (termination, iterations, final_cost)
    assert summary["num_successful_steps"] >= 2
    assert poses[:S][submap_order].tobytes() == p.submaps.tobytes() and poses[S:][node_order].tobytes() == p.nodes.tobytes()
    assert poses[S:].tobytes() != g.nodes.tobytes()
    if frozen == 1:
        assert poses[1:S:2].tobytes() == g.submaps[1::2].tobytes() and poses[S + 1::2].tobytes() == g.nodes[1::2].tobytes()
