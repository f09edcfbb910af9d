"""GPU tests of the pose graph solve's landmark observations (include/dliom.h dliom_pose_graph_landmarks:
LandmarkCostFunction3D, promoted nodes and landmarks in the dense reduced system) against the CPU model (tests/cpp/
pose_graph_model.cc).  The bars are those of tests/test_gpu_pose_graph_terms.py: `evaluate` 1e-9 relative; `step`
within 10 x the difference between the model's own two linear solvers on the same case; `solve` with equal termination,
iteration counts and accept / reject sequences, poses within 1e-6 m and 1e-6 rad -- the landmarks' included -- and costs
within 1e-9 relative."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
import pose_graph_landmarks_common as lc  # noqa: E402
import pose_graph_terms_common as tc  # noqa: E402

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


def promoted_nodes(g):
    """the non-constant nodes that a remaining observation names"""
    out = set()
    for o in g.observations:
        if g.node_constant[o["prev_node"]] and g.node_constant[o["next_node"]] and g.landmark_constant[o["landmark"]]:
            continue
        out |= {int(n) for n in (o["prev_node"], o["next_node"]) if not g.node_constant[n]}
    return sorted(out)


def reduced_dimension(g, model_columns):
    """The model counts every column; the device's system has none of the eliminated nodes' (every node of these graphs has
    a constraint)."""
    eliminated = int((g.node_constant == 0).sum()) - len(promoted_nodes(g))
    return model_columns - (5 if g.fix_z else 6) * eliminated


@pytest.mark.parametrize("fix_z", [False, True])
def test_evaluate(dl, ctx, model, fix_z):
    """4 submaps, 40 nodes, 3 landmarks, 14 observations that hold every branch by construction (tests/
    test_pose_graph_landmarks_host.py::test_the_evaluate_case_holds_every_branch asserts that they do).  A frozen trajectory's
    nodes are constant and so never promoted; "a promoted node on a frozen trajectory" is covered by the pair (13, 14) that
    straddles the frozen trajectory's end -- a constant prev, a promoted next -- and by the pair (2, 3) of two constant nodes
    under a free landmark."""
    exe, d = model
    g = lc.evaluate_graph(fix_z)
    cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
    got_cost, got_residuals, got_gradient = g.device(dl, ctx).evaluate()
    print("cost", abs(got_cost - cost) / cost, "residuals", relative(got_residuals, residuals), "gradient", relative(got_gradient, gradient))
    assert abs(got_cost - cost) <= 1e-9 * cost
    assert relative(got_residuals, residuals) <= 1e-9 and relative(got_gradient, gradient) <= 1e-9
    # every observation on its own, the fixed one included
    for i in range(len(g.observations)):
        assert relative(got_residuals[len(g.constraints) + i], residuals[len(g.constraints) + i]) <= 1e-9, i
    assert np.array_equal(got_gradient == 0, gradient == 0)  # the same slots are outside the problem
    S, N = len(g.submaps), len(g.nodes)
    landmarks, promoted = got_gradient[S + N:], got_gradient[S:S + N][promoted_nodes(g)]
    assert np.all(landmarks[:2] != 0) and np.all(landmarks[2] == 0)  # a landmark's z stays a column under fix_z
    assert np.all(promoted[:, [0, 1, 3, 4, 5]] != 0) and np.all(promoted[:, 2] == 0) == fix_z


@pytest.mark.parametrize("name", list(lc.STEP_CASES))
def test_step(dl, ctx, model, name):
    """Reduced dimensions 256 (one workgroup) and 260 (blocked) reached through promoted nodes and landmarks, and a small
    system whose panel boundaries at 32 and 64 lie inside the promoted nodes' columns."""
    exe, d = model
    pairs, landmarks, fix_z, dimension = lc.STEP_CASES[name]
    g = lc.boundary_graph(pairs, landmarks, fix_z)
    qr, eliminated = pc.model_step(exe, g, d, pc.SPARSE_QR), pc.model_step(exe, g, d, pc.ELIMINATED)
    cpu = relative(eliminated["delta"], qr["delta"])
    delta, change, got_dimension = g.device(dl, ctx).step(1e4)
    got = relative(delta, qr["delta"])
    print(name, "reduced dimension", got_dimension, "cpu solvers differ by", cpu, "device from QR", got, "model cost change",
          abs(change - qr["model_cost_change"]) / qr["model_cost_change"])
    assert got_dimension == dimension == reduced_dimension(g, qr["columns"])
    submap_columns = 12 if fix_z else 14
    assert submap_columns < 32 and submap_columns + (5 if fix_z else 6) * 2 * pairs > 64  # the panels' boundaries: promoted columns
    assert cpu > 0
    assert got <= 10 * cpu
    assert abs(change - qr["model_cost_change"]) <= 1e-9 * qr["model_cost_change"]
    assert np.array_equal(delta == 0, qr["delta"] == 0)


def solve_both(dl, ctx, exe, d, g):
    p = g.device(dl, ctx)
    return pc.model_solve(exe, g, d), p, p.solve()


def assert_equal_solves(name, g, want, p, summary):
    got = np.concatenate([p.submaps, p.nodes, p.fixed_frames, p.landmarks])
    model_poses = np.concatenate([want["submaps"], want["nodes"], want["frames"], want["landmarks"]])
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
            g = lc.CASES[name](exe, d)
            out[name] = (g,) + solve_both(dl, ctx, exe, d, g)
        return out[name]
    return get


@pytest.mark.parametrize("name", list(lc.CASES))
def test_solve(solved, name):
    g, want, p, summary = solved(name)
    assert_equal_solves(name, g, want, p, summary)
    assert summary["reduced_dimension"] == reduced_dimension(g, want["columns"])
    assert (0 in summary["steps"]) == (name in lc.REJECTING)
    if g.landmark_constant.all():
        assert p.landmarks.tobytes() == g.landmarks.tobytes()
    else:
        assert not np.any(np.all(p.landmarks == g.landmarks, axis=1))  # every landmark moved


def test_one_landmark_closes_the_loop(dl, ctx, model, solved):
    """A single landmark seen at both ends of a drifting trajectory pulls the summed node error below the solve without it --
    on the model, and the device equals the model in both runs."""
    exe, d = model
    with_it, without, truth = lc.loop_pair()
    _, want, p, summary = solved("s6_n120_one_landmark_closes_the_loop")
    want0, p0, summary0 = solve_both(dl, ctx, exe, d, without)
    assert_equal_solves("without the landmark", without, want0, p0, summary0)
    errors = [(tc.node_error(truth, w["nodes"]), tc.node_error(truth, q.nodes)) for w, q in ((want, p), (want0, p0))]
    print("node error (model, device) with and without the landmark:", errors)
    assert errors[0][0] < errors[1][0] and errors[0][1] < errors[1][1]


@pytest.mark.parametrize("name", ["s6_n120_landmarks_frames_loss", "s6_n120_landmarks_rejects_30"])
def test_two_solves_with_landmarks_are_bit_identical(dl, ctx, solved, name):
    g, _, p, summary = solved(name)
    again = g.device(dl, ctx)
    stats = ctx.memory_stats()
    summary2 = again.solve()
    assert ctx.memory_stats() == stats
    assert again.submaps.tobytes() == p.submaps.tobytes() and again.nodes.tobytes() == p.nodes.tobytes()
    assert again.fixed_frames.tobytes() == p.fixed_frames.tobytes() and again.landmarks.tobytes() == p.landmarks.tobytes()
    assert (summary2["final_cost"], summary2["initial_cost"], summary2["steps"]) == (summary["final_cost"], summary["initial_cost"], summary["steps"])


@pytest.mark.parametrize("name", ["reduces_noise", "s44_n900_nonmonotonic_50"])
def test_entry_points_are_bit_identical(dl, ctx, model, name):
    """The old entry point, the new one with NULL and the new one with an empty struct (s44: 260 columns, the blocked
    factorisation)."""
    exe, d = model
    g = lc.Graph(pc.CASES[name](exe, d))
    results = []
    for entry in ("plain", "landmarks_null", "landmarks_empty"):
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
    base, truth, _ = tc.synthetic(3, 12, 1, seed=1)
    good = lc.with_landmarks(base, truth, lc.some_landmarks(2, 1), [(0, 2, 0.5), (1, 8, 0.25), (0, 9, 0.75)], seed=1)

    def refused(graph, status):
        p = graph.device(dl, ctx)
        before = (p.submaps.copy(), p.nodes.copy(), p.landmarks.copy())
        for call in (p.solve, p.evaluate, p.step):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == status
        for a, b in zip(before, (p.submaps, p.nodes, p.landmarks)):
            assert np.array_equal(a, b, equal_nan=True)

    def edited(key=None, index=None, value=None):
        g = lc.Graph(good, good.landmarks.copy(), good.landmark_constant.copy(), good.observations.copy())
        if key is not None:
            g.observations[key][index] = value
        return g
    refused(edited("landmark", 1, 2), dl.ERR_INVALID_ARGUMENT)      # a landmark index out of range
    refused(edited("landmark", 1, -1), dl.ERR_INVALID_ARGUMENT)
    refused(edited("prev_node", 0, 12), dl.ERR_INVALID_ARGUMENT)    # a node index out of range
    refused(edited("next_node", 2, -1), dl.ERR_INVALID_ARGUMENT)
    refused(edited("next_node", 0, 2), dl.ERR_INVALID_ARGUMENT)     # prev_node == next_node
    for value in (np.nan, np.inf):
        refused(edited("interpolation_parameter", 1, value), dl.ERR_SOLVER)
    refused(edited("translation_weight", 2, np.nan), dl.ERR_SOLVER)
    refused(edited("rotation_weight", 0, -np.inf), dl.ERR_SOLVER)
    nan = edited()
    nan.observations["landmark_to_tracking"][1, 4] = np.nan
    refused(nan, dl.ERR_SOLVER)
    nan = edited()
    nan.landmarks[1, 0] = np.nan
    refused(nan, dl.ERR_SOLVER)

    # a positive count with a NULL array: the binding cannot say that, so the struct is patched
    class Patched(dl.PoseGraph):
        def _call(self, name, *rest):
            landmarks = dl.PoseGraphLandmarks(self.counts[0], self.pointers[0], None, self.counts[1], self.pointers[1])
            dl._check(getattr(self._L, "dliom_pose_graph_%s_landmarks" % name)(self.ctx.h, dl.C.byref(self.options), *self._graph(),
                                                                               None, dl.C.byref(landmarks), *rest), name)
    for counts, keep in (((2, 0), None), ((2, 3), 0), ((-1, 0), None), ((0, -1), None)):
        p = Patched(ctx, good.submaps, good.nodes, good.constraints, landmarks=good.landmarks, landmark_observations=good.observations)
        p.counts = counts
        p.pointers = [None, None]
        if keep is not None:
            p.pointers[keep] = dl._p(p.landmarks, dl._f64p)
        for call in (p.solve, p.evaluate, p.step):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == dl.ERR_INVALID_ARGUMENT
    # too many columns: 1 366 promoted nodes of six columns are 8 196 > 8 192
    many = 1366
    big, big_truth, _ = tc.synthetic(3, many, 0, seed=2)
    frozen_submaps = pc.Graph(big.submaps, big.nodes, big.constraints, np.ones(3, np.uint8), big.node_constant)
    sightings = [(0, i, 0.5) for i in range(0, many, 2)]
    too_large = lc.with_landmarks(frozen_submaps, big_truth, lc.some_landmarks(1, 2), sightings, seed=2, start="truth", landmark_constant=[1])
    refused(too_large, dl.ERR_TOO_LARGE)
    L.dliom_ctx_read_backs(ctx.h, dl.C.byref(n))
    assert n.value == read_backs and ctx.memory_stats() == stats
    # the unedited graph is accepted: 2 + 6 + 6 of the submaps, the six nodes 2, 3, 8, 9, 9, 10 -> five, two landmarks
    assert good.device(dl, ctx).step(1e4)[2] == 14 + 6 * 5 + 6 * 2


@pytest.mark.parametrize("frozen", [-1, 1])
def test_adapter(dl, ctx, tmp_path, frozen):
    """tests/cpp/pose_graph_landmarks_adapter.cc -- OptimizationProblem3D::Solve with options.use_landmarks on two trajectories
    and a third of one node -- against the Python binding fed by pose_graph_landmarks_common.adapter_compact, bit for bit.
    Like tests/test_gpu_pose_graph.py::test_adapter a SELF-COMPARISON of two routes into one entry point: it checks the
    adapter's host steps and where its results go, not the solve."""
    import subprocess
    exe = str(tmp_path / "pose_graph_landmarks_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "pose_graph_landmarks_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    g, _, spec = lc.adapter_case()
    S, N = len(g.submaps), len(g.nodes)
    src, dst = str(tmp_path / "graph.bin"), str(tmp_path / "adapter.bin")
    lc.adapter_write(src, g, spec, frozen, True)
    subprocess.check_call([exe, src, dst])
    data = open(dst, "rb").read()
    used, starts, constant, observations = lc.adapter_compact(dl.initial_landmark_pose, g.nodes, spec, frozen, True)
    record = np.dtype([("poses", "<f8", (S + N, 7)), ("count", "<i4"), ("landmarks", "<f8", (len(used), 7)), ("termination", "<i4"),
                       ("iterations", "<i4"), ("final_cost", "<f8")])
    assert len(data) == record.itemsize
    got = np.frombuffer(data, dtype=record)[0]
    # the same graph in the adapter's MapById order: trajectory 0 (even inputs), trajectory 1 (odd inputs), the extra node
    submap_order = np.r_[np.arange(0, S, 2), np.arange(1, S, 2)]
    node_order = np.array(lc.adapter_node_order(N, True))
    constraints = g.constraints.copy()
    constraints["submap"] = np.argsort(submap_order)[g.constraints["submap"]]
    constraints["node"] = np.argsort(node_order)[g.constraints["node"]]
    nodes = np.concatenate([g.nodes, [[0.0, 0, 0, 1, 0, 0, 0]]])[node_order]
    on_frozen = lambda order: (order % 2 == frozen).astype(np.uint8) if frozen >= 0 else None  # noqa: E731
    node_constant = on_frozen(node_order)
    if node_constant is not None:
        node_constant[-1] = 0  # the extra node is trajectory 2's
    p = dl.PoseGraph(ctx, g.submaps[submap_order], nodes, constraints, on_frozen(submap_order), node_constant, 0, g.fix_z,
                     g.nonmonotonic, g.max_iterations, landmarks=starts, landmark_constant=constant, landmark_observations=observations)
    summary = p.solve()
    print("frozen", frozen, summary["termination_type"], summary["num_iterations"], summary["steps"], summary["final_cost"])
    assert (summary["termination_type"], summary["num_iterations"], summary["final_cost"]) == (
        got["termination"], got["iterations"], got["final_cost"])
    assert got["poses"][:S][submap_order].tobytes() == p.submaps.tobytes()
    assert got["poses"][S:][node_order[:-1]].tobytes() == p.nodes[:-1].tobytes()
    assert got["count"] == len(used) and got["landmarks"].tobytes() == p.landmarks.tobytes()  # "landmark%03d": the map's order
    assert summary["num_successful_steps"] >= 2
    assert (p.landmarks.tobytes() == starts.tobytes()) == (frozen >= 0)
