"""The pose graph solve's landmark observations without a GPU: the CPU model (tests/cpp/pose_graph_model.cc) on graphs
with LandmarkCostFunction3D against the reference's own known answer, against hand computations and an independent
minimiser; the honesty of the parity cases; the host helper dliom_pose_graph_initial_landmark_pose; and the host
structure builder (d-liom_amd/csrc/pose_graph_structure.h) on promoted nodes under sanitisers, as a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import least_squares

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
import pose_graph_landmarks_common as lc  # noqa: E402
import pose_graph_terms_common as tc  # noqa: E402
from pose_graph_common import synth  # noqa: E402
from test_pose_graph_host import numpy_residual  # noqa: E402


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph_model")
    return pc.build_model(d), d


def test_the_references_known_answer(model):
    """landmark_cost_function_3d_test.cc's SmokeTest: residuals (1, 0, 0, 0, 0, 0) exactly."""
    exe, d = model
    identity = [1.0, 0.0, 0.0, 0.0]
    nodes = np.array([[0.0, 0.0, 0.0] + identity, [2.0, 2.0, 2.0] + identity])
    base = pc.Graph(np.zeros((0, 7)), nodes, np.zeros(0, pc.CONSTRAINT), gravity=-1)
    rows = [(0, 0, 1, 0.5, np.array([1.0, 1.0, 1.0] + identity), 1.0, 2.0)]
    g = lc.Graph(base, np.array([[1.0, 2.0, 2.0] + identity]), None, lc.rows_to_observations(rows))
    cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
    assert residuals.tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]] and cost == 0.5
    assert lc.landmark_residual(g.observations[0], nodes[0], nodes[1], g.landmarks[0]).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # d e0 / d (prev.x, next.x, landmark.x) = (1 - t, t, -1), times e0 = 1
    assert np.allclose(gradient[:, 0], [0.5, 0.5, -1.0], rtol=0, atol=1e-15)


def _promoted(g):
    """the nodes a remaining observation names and that are not constant"""
    out = set()
    for o in g.observations:
        blocks = [g.node_constant[o["prev_node"]], g.node_constant[o["next_node"]], g.landmark_constant[o["landmark"]]]
        if all(blocks):
            continue
        out |= {int(n) for n in (o["prev_node"], o["next_node"]) if not g.node_constant[n]}
    return sorted(out)


def test_the_evaluate_case_holds_every_branch(model):
    """tests/test_gpu_pose_graph_landmarks.py::test_evaluate's graph by construction, the model's residuals against the
    hand-written ones, and the zero pattern of its gradient."""
    exe, d = model
    for fix_z in (False, True):
        g = lc.evaluate_graph(fix_z)
        assert (len(g.submaps), len(g.nodes), len(g.landmarks), len(g.observations)) == (4, 40, 3, 14)
        cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
        C, S, N = len(g.constraints), len(g.submaps), len(g.nodes)
        cosines = [lc.slerp_scales(g.nodes[o["prev_node"], 3:], g.nodes[o["next_node"], 3:], 0.5)[2] for o in g.observations]
        assert abs(cosines[0]) >= 1 - 1e-5                                   # the linear branch
        assert 0 < cosines[1] < 0.6                                          # the slerp branch, more than 100 degrees apart
        assert cosines[2] < -0.9                                             # next.q negated
        assert sorted(g.observations["interpolation_parameter"])[0] == 0.0 and sorted(g.observations["interpolation_parameter"])[-1] == 1.0
        assert sorted(set(g.constraints["submap"][g.constraints["node"] == 26])) == [1, 2]
        assert sorted(set(g.observations["landmark"][(g.observations["prev_node"] == 26) | (g.observations["next_node"] == 26)])) == [0, 1]
        assert g.node_constant[13] and not g.node_constant[14] and g.landmark_constant.tolist() == [0, 0, 1]
        total = 0.0
        for c, k in enumerate(g.constraints):
            total += 0.5 * (numpy_residual(g.submaps[k["submap"]], g.nodes[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"]) ** 2).sum()
        for i, o in enumerate(g.observations):
            r = lc.landmark_residual(o, g.nodes[o["prev_node"]], g.nodes[o["next_node"]], g.landmarks[o["landmark"]])
            assert np.allclose(residuals[C + i], r, rtol=1e-9, atol=1e-9), i
            total += 0.5 * (r ** 2).sum()
        assert abs(cost - total) <= 1e-12 * cost
        promoted = _promoted(g)
        assert promoted == [14, 16, 17, 18, 19, 20, 21, 25, 26, 27, 30, 31, 33, 34, 35, 36, 38, 39]
        assert np.all(gradient[S + N:S + N + 2] != 0) and np.all(gradient[S + N + 2] == 0)  # six columns also under fix_z
        assert np.all(gradient[S:S + N][promoted][:, 2] == 0) == fix_z and np.all(gradient[S:S + N][promoted][:, [0, 1, 3, 4, 5]] != 0)
        assert np.all(gradient[S:S + 14] == 0)


class Unknowns:
    """The free blocks as one vector: the gravity-aligned first submap's two rotation columns, six a further submap, a node
    and a landmark (translation added, exp(d) (x) q)."""

    def __init__(self, g):
        self.g = g
        assert not g.submap_constant.any() and not g.node_constant.any() and not g.landmark_constant.any() and not g.fix_z
        assert g.gravity == 0 and len(g.frames) == 0 and g.huber_scale == 0
        self.size = 2 + 6 * (len(g.submaps) - 1 + len(g.nodes) + len(g.landmarks))
        self.is_angle = np.array([1, 1] + [0, 0, 0, 1, 1, 1] * (len(g.submaps) - 1 + len(g.nodes) + len(g.landmarks)), bool)

    def poses(self, p):
        g = self.g
        s, n, l = g.submaps.copy(), g.nodes.copy(), g.landmarks.copy()
        s[0, 3:] = synth._quat_mul(s[0, 3:], synth._quat_of([p[0], p[1], 0.0]))
        at = 2
        for arr, first in ((s, 1), (n, 0), (l, 0)):
            for i in range(first, len(arr)):
                arr[i, :3] += p[at:at + 3]
                arr[i, 3:] = synth._quat_mul(synth._quat_of(p[at + 3:at + 6]), arr[i, 3:])
                at += 6
        assert at == self.size
        return s, n, l

    def blocks(self, p):
        g = self.g
        s, n, l = self.poses(p)
        rows = [numpy_residual(s[k["submap"]], n[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"]) for k in g.constraints]
        rows += [lc.landmark_residual(o, n[o["prev_node"]], n[o["next_node"]], l[o["landmark"]]) for o in g.observations]
        return np.array(rows)

    def cost(self, p):
        return 0.5 * (self.blocks(p) ** 2).sum()


def small_graph(seed):
    base, truth, _ = tc.synthetic(3, 12, 0, seed=seed, max_iterations=200)
    return lc.with_landmarks(base, truth, lc.some_landmarks(2, seed), [(0, 1, 0.3), (1, 4, 0.6), (0, 8, 0.5), (1, 10, 0.0)], seed=seed)


def test_independent_minimum(model):
    """The model's final cost against scipy.optimize.least_squares on hand-written residuals; the bar of
    tests/test_pose_graph_host.py::test_independent_minimum: Ceres stops early (function tolerance 1e-6), so the model may
    not undercut the converged minimum and lies within 1e-4 of it."""
    exe, d = model
    g = small_graph(81)
    u = Unknowns(g)
    for solver in (pc.ELIMINATED, pc.SPARSE_QR):
        got = pc.model_solve(exe, g, d, solver)
        if solver == pc.ELIMINATED:
            sol = least_squares(lambda p: u.blocks(p).reshape(-1), np.zeros(u.size), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
            cost_min = 0.5 * (sol.fun ** 2).sum()
        print("model", got["final_cost"], "scipy", cost_min, got["iterations"])
        assert got["columns"] == len(sol.x)
        assert got["final_cost"] >= cost_min * (1.0 - 1e-9)
        assert got["final_cost"] <= cost_min * (1.0 + 1e-4)
        assert got["initial_cost"] > 10 * got["final_cost"]
        assert got["landmarks"].tobytes() != g.landmarks.tobytes()


def test_gradient_by_central_differences(model):
    """The model's J^T r, slot by slot -- promoted nodes and landmarks among them --, against central differences of the
    hand-written 1/2 sum r^2."""
    exe, d = model
    g = small_graph(82)
    cost, residuals, gradient, columns = pc.model_evaluate(exe, g, d)
    u = Unknowns(g)
    assert columns == u.size and abs(cost - u.cost(np.zeros(u.size))) <= 1e-9 * cost
    want = np.concatenate([gradient[0, 3:5], gradient[1:].reshape(-1)])  # no fixed frame: submaps, nodes, landmarks
    h = 1e-6
    scale = np.abs(want).max()
    worst = 0.0
    for i in range(u.size):
        e = np.zeros(u.size)
        e[i] = h
        numeric = (u.cost(e) - u.cost(-e)) / (2 * h) * (2.0 if u.is_angle[i] else 1.0)
        worst = max(worst, abs(numeric - want[i]) / scale)
    print("gradient: worst difference", worst, "of", scale)
    assert worst <= 1e-6


@pytest.mark.parametrize("name", list(lc.CASES))
def test_parity_cases_are_honest(model, name):
    """tests/test_pose_graph_terms_host.py::test_parity_cases_are_honest with one more margin: no observation's |cos theta|
    within 1e-6 of 1 - 1e-5, and no cos theta within 1e-6 of 0, at any evaluated point; for the eliminated normal equations
    with the promoted layout and the structured QR, within 1e-8 of each other and with equal step sequences."""
    exe, d = model
    g = lc.CASES[name](exe, d)
    a = pc.model_solve(exe, g, d, pc.ELIMINATED)
    b = pc.model_solve(exe, g, d, pc.SPARSE_QR)
    difference = max(np.abs(a[key] - b[key]).max(initial=0.0) for key in ("nodes", "submaps", "frames", "landmarks"))
    print(name, a["termination"], a["iterations"], a["steps"], a["quality_margin"], a["tolerance_margin"], a["loss_margin"],
          a["clamp_margin"], a["slerp_margin"], "solvers differ by", difference)
    assert a["termination"] in (0, 1) and a["successful"] >= 2 and 2 not in a["steps"]
    assert (0 in a["steps"]) == (name in lc.REJECTING)
    for r in (a, b):
        assert min(r["quality_margin"], r["tolerance_margin"], r["loss_margin"], r["clamp_margin"], r["slerp_margin"]) > 1e-6
    assert (a["termination"], a["iterations"], a["steps"], a["rises"], a["clamped_steps"]) == (
        b["termination"], b["iterations"], b["steps"], b["rises"], b["clamped_steps"])
    assert difference <= 1e-8
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-8 * a["final_cost"]


def test_the_step_cases_are_honest(model):
    """The step cases' two linear solvers agree (their difference is the bar of the device's step test) and the evaluated
    point is away from the slerp's branch points."""
    exe, d = model
    for name, (pairs, landmarks, fix_z, _) in lc.STEP_CASES.items():
        g = lc.boundary_graph(pairs, landmarks, fix_z)
        a, b = pc.model_step(exe, g, d, pc.SPARSE_QR), pc.model_step(exe, g, d, pc.ELIMINATED)
        difference = np.abs(a["delta"] - b["delta"]).max()
        margin = pc.model_solve(exe, lc.Graph(g, g.landmarks, g.landmark_constant, g.observations, max_iterations=0), d)["slerp_margin"]
        print(name, "solvers differ by", difference, "of", np.abs(a["delta"]).max(), "slerp margin", margin)
        assert difference <= 1e-8 and margin > 1e-6


def test_the_cases_cover_what_they_name(model):
    exe, d = model
    g = lc.CASES["s3_n30_initial_landmark_pose"](exe, d)
    first = g.observations[np.flatnonzero(g.observations["landmark"] == 1)[0]]
    want = lc.initial_landmark_pose(g.nodes[first["prev_node"]], g.nodes[first["next_node"]], first["interpolation_parameter"],
                                    first["landmark_to_tracking"])
    assert g.landmarks[1].tobytes() == want.tobytes()
    # a landmark that starts at its first observation has a zero residual there
    assert np.abs(lc.landmark_residual(first, g.nodes[first["prev_node"]], g.nodes[first["next_node"]], want)).max() < 1e-9
    g = lc.CASES["s4_n40_frozen_landmarks"](exe, d)
    assert g.landmark_constant.all() and g.node_constant.any() and not g.node_constant.all()
    solved = pc.model_solve(exe, g, d)
    assert solved["landmarks"].tobytes() == g.landmarks.tobytes()
    assert solved["nodes"][g.node_constant != 0].tobytes() == g.nodes[g.node_constant != 0].tobytes()
    g = lc.CASES["s6_n120_landmarks_frames_loss"](exe, d)
    assert len(g.frames) > 0 and g.huber_scale > 0 and g.inter_submap.any() and len(g.observations) > 0
    # one landmark closes the loop, on the model (the device's run is tests/test_gpu_pose_graph_landmarks.py's)
    with_it, without, truth = lc.loop_pair()
    errors = [tc.node_error(truth, pc.model_solve(exe, graph, d)["nodes"]) for graph in (with_it, without)]
    print("node errors with and without the landmark", errors)
    assert errors[0] < errors[1]


def test_initial_landmark_pose_helper():
    """dliom_pose_graph_initial_landmark_pose (host code of the library) against the restatement in numpy, on the slerp
    branch, the linear branch and a negated quaternion."""
    import __graft_entry__
    dl = __graft_entry__.build()
    rng = np.random.RandomState(7)
    worst = 0.0
    for case in range(12):
        a = np.concatenate([rng.uniform(-3, 3, 3), synth._quat_of(rng.uniform(-1.5, 1.5, 3))])
        b = np.concatenate([rng.uniform(-3, 3, 3), synth._quat_of(rng.uniform(-1.5, 1.5, 3))])
        if case % 3 == 1:
            b[3:] = a[3:]
        if case % 3 == 2:
            b[3:] = -b[3:]
        z = np.concatenate([rng.uniform(-1, 1, 3), synth._quat_of(rng.uniform(-1.5, 1.5, 3))])
        t = [0.0, 1.0, 0.37, 0.81][case % 4]
        got, want = dl.initial_landmark_pose(a, b, t, z), lc.initial_landmark_pose(a, b, t, z)
        worst = max(worst, np.abs(got - want).max())
    print("worst difference", worst)
    assert worst <= 1e-14


def test_structure_builder_under_sanitizers(model, tmp_path):
    """tests/cpp/pose_graph_structure_check.cc, a stand-alone program built with -fsanitize=address,undefined: the case
    lists with and without landmarks, promotion and columns under fix_z, a landmark that only constant nodes see, an
    observation with all six blocks constant, the column cap and bad indices."""
    exe, d = model
    check = pc.build_structure_check(tmp_path)
    graphs = [make(exe, d) for make in lc.CASES.values()]
    without = [lc.Graph(make(exe, d)) for make in tc.CASES.values()] + [lc.Graph(pc.branches_graph(True))]
    named = [lc.evaluate_graph(False), lc.evaluate_graph(True)] + [lc.boundary_graph(*k[:3]) for k in lc.STEP_CASES.values()]
    base, truth, _ = tc.synthetic(3, 12, 0, seed=1)
    constant_nodes = np.zeros(12, np.uint8)
    constant_nodes[[4, 5]] = 1
    frozen_pair = pc.Graph(base.submaps, base.nodes, base.constraints, base.submap_constant, constant_nodes)
    one = lc.with_landmarks(frozen_pair, truth, lc.some_landmarks(2, 1), [(0, 4, 0.5), (1, 8, 0.5)], seed=1)
    named.append(one)                                                                        # landmark 0: only constant nodes see it
    named.append(lc.Graph(frozen_pair, one.landmarks, [1, 0], one.observations))             # ... and constant itself: all six fixed
    named.append(lc.Graph(frozen_pair, one.landmarks, None, None))                           # landmarks nothing observes
    paths = []
    for i, g in enumerate(graphs + without + named):
        paths.append(str(tmp_path / ("graph%d.bin" % i)))
        pc._write(g, paths[-1], 0, 0, 1e4)
    out = subprocess.check_output([check] + paths).decode().splitlines()
    print("\n".join(out))
    assert len(out) == len(paths) and all(" ok columns " in line for line in out)
    fields = [pc.structure_check_fields(line) for line in out[len(graphs) + len(without):]]
    columns, direct, promoted = [f["columns"] for f in fields], [f["direct"] for f in fields], [f["promoted"] for f in fields]
    # the evaluate graph: three free submaps, 18 promoted nodes, two free landmarks
    assert columns[:2] == [18 + 18 * 6 + 12, 15 + 18 * 5 + 12] and promoted[:2] == [18, 18]
    assert columns[2:5] == [k[3] for k in lc.STEP_CASES.values()] and promoted[2:5] == [44, 40, 10]
    # one's submaps: 2 + 6 + 6; landmark 0 seen from constant nodes only: six columns, nothing promoted for it
    assert columns[5:] == [14 + 2 * 6 + 12, 14 + 2 * 6 + 6, 14] and promoted[5:] == [2, 2, 0]
    assert direct[5] == direct[6] > 0 and direct[7] == 0
    # the cap: 1 366 promoted nodes of six columns are 8 196 > 8 192 columns
    many = 1366
    nodes = np.tile(base.nodes[:1], (many, 1))
    rows = [(0, i, i + 1, 0.5, base.nodes[0], 1.0, 1.0) for i in range(0, many, 2)]
    big = lc.Graph(pc.Graph(base.submaps[:0], nodes, base.constraints[:0], gravity=-1), one.landmarks[:1], [1], lc.rows_to_observations(rows))
    pc._write(big, paths[0], 0, 0, 1e4)
    assert subprocess.check_output([check, paths[0]]).decode().split()[-2:] == ["status", "2"]
    big.observations = big.observations[:-1]                                                 # 1 364 promoted nodes fit
    pc._write(big, paths[0], 0, 0, 1e4)
    assert subprocess.check_output([check, paths[0]]).decode().split()[1:4] == ["ok", "columns", str(6 * 1364)]
    for key, index, value in (("landmark", 0, 2), ("landmark", 1, -1), ("prev_node", 0, 12), ("next_node", 1, -1), ("next_node", 0, 4)):
        bad = lc.Graph(frozen_pair, one.landmarks, None, one.observations.copy())
        bad.observations[key][index] = value
        pc._write(bad, paths[0], 0, 0, 1e4)
        assert subprocess.check_output([check, paths[0]]).decode().split()[-2:] == ["status", "1"], (key, index, value)


@pytest.mark.parametrize("frozen", [-1, 1])
def test_the_adapters_host_steps(tmp_path, frozen):
    """OptimizationProblem3D::CompactLandmarks (dliom_cartographer.h, options.use_landmarks) without a context against the
    restatement of optimization_problem_3d.cc:124-186 in pose_graph_landmarks_common.adapter_compact, bit for bit, on two
    trajectories and a third of one node: an observation before the first node, at the first node's time, behind the last
    node, on a trajectory of one node and on one without nodes; a landmark none of whose observations is used; and, with a
    frozen trajectory, every landmark constant and those without a global pose left out."""
    import __graft_entry__
    dl = __graft_entry__.build()
    exe = str(tmp_path / "pose_graph_landmarks_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "pose_graph_landmarks_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    base, _, spec = lc.adapter_case()
    src, dst = str(tmp_path / "graph.bin"), str(tmp_path / "blocks.bin")
    lc.adapter_write(src, base, spec, frozen, True)
    subprocess.check_call([exe, "--host", src, dst])
    data = open(dst, "rb").read()
    count, rows = np.frombuffer(data, "<i4", 2)
    used, starts, constant, observations = lc.adapter_compact(dl.initial_landmark_pose, base.nodes, spec, frozen, True)
    print("frozen", frozen, "landmarks", used, "observations", len(observations), observations["interpolation_parameter"])
    if frozen < 0:
        assert used == [0, 1, 3] and len(observations) == 3 + 3 + 2
        first = observations[0]
        assert (first["prev_node"], first["next_node"], first["interpolation_parameter"]) == (0, 1, 0.0)  # nodes 0 and 2 of the file
        assert not constant.any()
    else:
        assert used == [1] and len(observations) == 3 and constant.all()
    assert (count, rows) == (len(used), len(observations))
    got_starts = np.frombuffer(data, "<f8", 7 * count, 8).reshape(-1, 7)
    got_constant = np.frombuffer(data, "<i4", count, 8 + 56 * count)
    record = np.dtype([("landmark", "<i4"), ("prev_node", "<i4"), ("next_node", "<i4"), ("interpolation_parameter", "<f8"),
                       ("landmark_to_tracking", "<f8", 7), ("translation_weight", "<f8"), ("rotation_weight", "<f8")])
    got = np.frombuffer(data, record, rows, 8 + 60 * count)
    assert len(data) == 8 + 60 * count + record.itemsize * rows
    assert got_starts.tobytes() == starts.tobytes() and list(got_constant) == list(constant)
    for name in record.names:
        assert got[name].tobytes() == np.ascontiguousarray(observations[name]).tobytes(), name
