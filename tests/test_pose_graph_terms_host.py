"""The pose graph solve's further terms without a GPU: the CPU model (tests/cpp/pose_graph_model.cc) on graphs with
fixed-frame pose constraints and the Huber loss against hand computations and against independent minimisers; the honesty
of the parity cases; and the host structure builder (d-liom_amd/csrc/pose_graph_structure.h) on fixed frames under
sanitisers, as a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import least_squares, minimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
import pose_graph_terms_common as tc  # noqa: E402
from pose_graph_common import synth  # noqa: E402
from test_pose_graph_host import numpy_residual  # noqa: E402


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph_model")
    return pc.build_model(d), d


# ---- independent mathematics: the unknowns as plain vectors, the residuals in numpy -------------------------------------------
def rho(s, a):
    """HuberLoss(a) at s = ||r||^2 (a == 0: TrivialLoss)."""
    return s if a == 0 or s <= a * a else 2 * a * np.sqrt(s) - a * a


class Unknowns:
    """The graph's free blocks as one vector: the gravity-aligned first submap's two rotation columns (x (x) exp([d0, d1,
    0])), six a further submap and a node (translation added, exp(d) (x) q), and a fixed frame's translation and its yaw
    as ONE SCALAR ANGLE (so none of YawOnlyQuaternionPlus's chart is used)."""

    def __init__(self, g):
        self.g = g
        assert not g.submap_constant.any() and not g.node_constant.any() and not g.fix_z and g.gravity == 0
        self.size = 2 + 6 * (len(g.submaps) - 1) + 6 * len(g.nodes) + 4 * len(g.frames)
        # which unknowns are angles: Ceres' tangent steps are HALF angles to first order ([cos |d|, sin |d| d / |d|], and
        # [sqrt(1 - d^2), 0, 0, d] with d = sin(yaw / 2)), so d cost / d step = 2 d cost / d angle there
        self.is_angle = np.array([1, 1] + [0, 0, 0, 1, 1, 1] * (len(g.submaps) - 1 + len(g.nodes)) + [0, 0, 0, 1] * len(g.frames), bool)

    def poses(self, p):
        g = self.g
        s, n, f = g.submaps.copy(), g.nodes.copy(), g.frames.copy()
        s[0, 3:] = synth._quat_mul(s[0, 3:], synth._quat_of([p[0], p[1], 0.0]))
        at = 2
        for arr, first in ((s, 1), (n, 0)):
            for i in range(first, len(arr)):
                arr[i, :3] += p[at:at + 3]
                arr[i, 3:] = synth._quat_mul(synth._quat_of(p[at + 3:at + 6]), arr[i, 3:])
                at += 6
        for i in range(len(f)):
            f[i, :3] += p[at:at + 3]
            f[i, 3:] = synth._quat_mul(synth._quat_of([0.0, 0.0, p[at + 3]]), f[i, 3:])
            at += 4
        assert at == self.size
        return s, n, f

    def blocks(self, p):
        """the residual blocks (C + CF, 6), uncorrected"""
        g = self.g
        s, n, f = self.poses(p)
        rows = [numpy_residual(s[k["submap"]], n[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"]) for k in g.constraints]
        rows += [numpy_residual(f[k["submap"]], n[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"])
                 for k in g.frame_constraints]
        return np.array(rows)

    def cost(self, p):
        g = self.g
        squared = (self.blocks(p) ** 2).sum(axis=1)
        lossy = np.concatenate([g.inter_submap, np.zeros(len(g.frame_constraints), np.uint8)])
        return 0.5 * sum(rho(s, g.huber_scale if tag else 0.0) for s, tag in zip(squared, lossy))

    def rooted(self, p):
        """r * sqrt(rho(s) / s) a block: a least-squares problem with the cost 1/2 sum rho(s)"""
        g = self.g
        r = self.blocks(p)
        lossy = np.concatenate([g.inter_submap, np.zeros(len(g.frame_constraints), np.uint8)])
        for c in np.flatnonzero(lossy):
            s = (r[c] ** 2).sum()
            if s > 0:
                r[c] *= np.sqrt(rho(s, g.huber_scale) / s)
        return r.reshape(-1)


def distance_bound(cost_min, jacobian):
    """How far a point whose cost exceeds the minimum by at most 1e-4 cost_min (the bar on the cost) can lie from the
    minimiser, in the unknowns' units (metres, radians): sqrt(2 excess / smallest eigenvalue of the Hessian J^T J)."""
    return np.sqrt(2 * 1e-4 * cost_min / np.linalg.eigvalsh(jacobian.T @ jacobian)[0])


def small_graph(huber_scale, seed):
    base, truth, inter = tc.synthetic(4, 24, 1, seed=seed, max_iterations=200)
    if huber_scale > 0:
        base, inter = tc.false_closure(base, inter, truth, 5.0, submap=1, node=20, seed=seed)
    return tc.with_fixed_frames(base, truth, [dict(origin=tc._yaw_pose([2.0, 1.0, 0.2], 0.5), nodes=list(range(0, 24, 2)))], seed=seed,
                                huber_scale=huber_scale, inter_submap=inter if huber_scale > 0 else None)


def test_independent_minimum_with_a_fixed_frame(model):
    """The model's final cost against scipy.optimize.least_squares on hand-written residuals with the fixed frame's yaw as
    a scalar unknown; the bar of tests/test_pose_graph_host.py::test_independent_minimum: Ceres stops early (function
    tolerance 1e-6), so the model may not undercut the converged minimum and lies within 1e-4 of it."""
    exe, d = model
    g = small_graph(0.0, 11)
    got = pc.model_solve(exe, g, d)
    u = Unknowns(g)
    sol = least_squares(lambda p: u.blocks(p).reshape(-1), np.zeros(u.size), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
    cost_min = 0.5 * (sol.fun ** 2).sum()
    print("model", got["final_cost"], "scipy", cost_min, got["iterations"])
    assert got["columns"] == len(sol.x)
    assert got["final_cost"] >= cost_min * (1.0 - 1e-9)
    assert got["final_cost"] <= cost_min * (1.0 + 1e-4)
    assert got["initial_cost"] > 10 * got["final_cost"]
    _, _, frames = u.poses(sol.x)
    bound = distance_bound(cost_min, sol.jac)
    print("fixed frame differs by", np.linalg.norm(frames[0, :3] - got["frames"][0, :3]), pc.rotation_angles(frames, got["frames"]).max(), "bound", bound)
    assert np.linalg.norm(frames[0, :3] - got["frames"][0, :3]) <= bound and pc.rotation_angles(frames, got["frames"]).max() <= bound


def test_independent_minimum_with_a_loss(model):
    """With a false closure under HuberLoss: scipy.optimize.minimize on the scalar 1/2 sum rho(s) reaches the model's final
    cost (the same bar) and its poses (distance_bound).  least_squares on r sqrt(rho(s) / s), whose squares sum to the same
    scalar, brings the start near enough for BFGS with differenced gradients to finish in seconds; the scalar is what is
    minimised last and what is compared."""
    exe, d = model
    g = small_graph(30.0, 12)
    got = pc.model_solve(exe, g, d)
    assert got["loss_margin"] < 1e300 and got["final_cost"] < got["initial_cost"]
    u = Unknowns(g)
    near = least_squares(u.rooted, np.zeros(u.size), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
    sol = minimize(u.cost, near.x, method="BFGS", options=dict(gtol=1e-3 * max(1.0, abs(u.cost(near.x))) * 1e-6, maxiter=50))
    cost_min = min(sol.fun, u.cost(near.x))
    best = sol.x if sol.fun <= u.cost(near.x) else near.x
    squared = (u.blocks(best) ** 2).sum(axis=1)[:len(g.constraints)][g.inter_submap != 0]
    assert (squared > g.huber_scale ** 2).any() and (squared < g.huber_scale ** 2).any()  # both regions of the loss
    print("model", got["final_cost"], "minimize", sol.fun, "least_squares", u.cost(near.x), got["iterations"])
    assert got["final_cost"] >= cost_min * (1.0 - 1e-9)
    assert got["final_cost"] <= cost_min * (1.0 + 1e-4)
    bound = distance_bound(cost_min, near.jac)
    s, n, f = u.poses(best)
    a, b = np.concatenate([s, n, f]), np.concatenate([got["submaps"], got["nodes"], got["frames"]])
    distance = max(np.linalg.norm(a[:, :3] - b[:, :3], axis=1).max(), pc.rotation_angles(a, b).max())
    print("poses differ by", distance, "bound", bound)
    assert distance <= bound


@pytest.mark.parametrize("huber_scale", [0.0, 30.0])
def test_gradient_by_central_differences(model, huber_scale):
    """The model's corrected J^T r, slot by slot, against central differences of the hand-written 1/2 sum rho(s)."""
    exe, d = model
    g = small_graph(huber_scale, 12)
    cost, residuals, gradient, columns = pc.model_evaluate(exe, g, d)
    u = Unknowns(g)
    assert columns == u.size and abs(cost - u.cost(np.zeros(u.size))) <= 1e-9 * cost
    S, N = len(g.submaps), len(g.nodes)
    # the model's slots in the unknowns' order: submap 0's two, the other submaps, the nodes, the fixed frame's four
    want = np.concatenate([gradient[0, 3:5], gradient[1:S + N].reshape(-1), gradient[S + N, :4]])
    assert np.all(gradient[S + N, 4:] == 0)
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


def test_the_evaluate_case_straddles_the_loss(model):
    """tests/test_gpu_pose_graph_terms.py::test_evaluate's graph: tagged constraints on both sides of huber_scale^2, none
    on the boundary; and the corrected residuals are the hand-written ones times sqrt(rho')."""
    exe, d = model
    for fix_z in (False, True):
        g = tc.evaluate_graph(fix_z, tc.EVALUATE_HUBER_SCALE)
        cost, residuals, gradient, _ = pc.model_evaluate(exe, g, d)
        b = g.huber_scale ** 2
        inside = outside = 0
        total = 0.0
        for c, k in enumerate(g.constraints):
            r = numpy_residual(g.submaps[k["submap"]], g.nodes[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"])
            s = (r ** 2).sum()
            if g.inter_submap[c]:
                assert abs(s - b) / b > 1e-6
                inside, outside = inside + (s < b), outside + (s > b)
                if s > b:
                    r = r * np.sqrt(g.huber_scale / np.sqrt(s))
                total += 0.5 * rho(s, g.huber_scale)
            else:
                total += 0.5 * s
            assert np.allclose(residuals[c], r, rtol=1e-9, atol=1e-9), c
        for c, k in enumerate(g.frame_constraints):
            r = numpy_residual(g.frames[k["submap"]], g.nodes[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"])
            total += 0.5 * (r ** 2).sum()
            assert np.allclose(residuals[len(g.constraints) + c], r, rtol=1e-9, atol=1e-9), c
        print("fix_z", fix_z, "tagged inside", inside, "outside", outside)
        assert inside >= 3 and outside >= 3
        assert abs(cost - total) <= 1e-12 * cost
        S, N = len(g.submaps), len(g.nodes)
        assert np.all(gradient[S + N:, :4] != 0) and np.all(gradient[S + N:, 4:] == 0)   # mask 15 also under fix_z
        assert np.all(gradient[S:S + N][g.node_constant == 0][:, 2] == 0) == fix_z


@pytest.mark.parametrize("name", list(tc.CASES))
def test_parity_cases_are_honest(model, name):
    """tests/test_pose_graph_host.py::test_parity_cases_are_honest with two more margins: no tagged constraint within 1e-6
    (relative) of the loss's boundary at any evaluated point, no yaw step within 1e-6 of the clamp; for the eliminated
    solver and the sparse QR, with equal step sequences between them."""
    exe, d = model
    g = tc.CASES[name](exe, d)
    a = pc.model_solve(exe, g, d, pc.ELIMINATED)
    print(name, a["termination"], a["iterations"], a["steps"], a["rises"], a["quality_margin"], a["tolerance_margin"],
          a["loss_margin"], a["clamp_margin"], a["clamped_steps"])
    assert a["termination"] in (0, 1) and a["successful"] >= 2 and 2 not in a["steps"]
    assert (0 in a["steps"]) == (name in tc.REJECTING) and (a["rises"] > 0) == (name in tc.RISING)
    assert (a["clamped_steps"] > 0) == (name in tc.CLAMPED)
    assert (a["loss_margin"] < 1e300) == (name in tc.LOSSY) and (a["clamp_margin"] < 1e300) == (len(g.frames) > 0)
    b = pc.model_solve(exe, g, d, pc.SPARSE_QR)
    for r in (a, b):
        assert min(r["quality_margin"], r["tolerance_margin"], r["loss_margin"], r["clamp_margin"]) > 1e-6
    assert (a["termination"], a["iterations"], a["steps"], a["rises"], a["clamped_steps"]) == (
        b["termination"], b["iterations"], b["steps"], b["rises"], b["clamped_steps"])
    for key in ("nodes", "submaps", "frames"):
        assert np.abs(a[key] - b[key]).max(initial=0.0) <= 1e-8


def test_the_cases_cover_what_they_name(model):
    exe, d = model
    g = tc.CASES["s4_n40_frame_on_frozen"](exe, d)
    on_frozen = g.frame_constraints["node"][g.frame_constraints["submap"] == 0]
    assert g.node_constant[on_frozen].all()  # a free block whose constraints touch only constant nodes
    solved = pc.model_solve(exe, g, d)
    assert solved["frames"][0].tobytes() != g.frames[0].tobytes()
    assert solved["nodes"][g.node_constant != 0].tobytes() == g.nodes[g.node_constant != 0].tobytes()
    g = tc.CASES["s3_n20_frame_from_mid_trajectory"](exe, d)
    assert g.frame_constraints["node"].min() == 9
    g = tc.CASES["s3_n20_clamped_yaw"](exe, d)
    z = g.frame_constraints[0]
    first = synth.pose7_compose(g.nodes[z["node"]], synth.pose7_inverse(z["zbar"]))
    assert 1.4 < abs(tc.get_yaw(synth._quat_mul(g.frames[0, 3:], first[3:] * [1, -1, -1, -1]))) < 1.8  # about 90 degrees off
    # the loss does its job, on the model (the device's run is tests/test_gpu_pose_graph_terms.py's)
    errors = {}
    for scale in (0.0, tc.LOSS_HUBER_SCALE):
        g, truth = tc.loss_pair(scale)
        errors[scale] = tc.node_error(truth, pc.model_solve(exe, g, d)["nodes"])
    print("node errors", errors)
    assert errors[tc.LOSS_HUBER_SCALE] < errors[0.0]


def test_structure_builder_under_sanitizers(model, tmp_path):
    """tests/cpp/pose_graph_structure_check.cc, a stand-alone program built with -fsanitize=address,undefined, on
    both case lists, the evaluate and step graphs and degenerate fixed frames."""
    exe, d = model
    check = pc.build_structure_check(tmp_path)
    graphs = [make(exe, d) for make in tc.CASES.values()] + [tc.Graph(make(exe, d)) for make in pc.CASES.values()]
    graphs += [tc.evaluate_graph(False, tc.EVALUATE_HUBER_SCALE), tc.evaluate_graph(True, 0.0), tc.Graph(pc.branches_graph(True))]
    graphs += [tc.boundary_graph(*k) for k in ((42, 2, False), (42, 3, False), (51, 1, True), (51, 2, True))]
    base, truth, _ = tc.synthetic(3, 12, 0, seed=1)
    one = tc.with_fixed_frames(base, truth, [dict(origin=tc._yaw_pose([1.0, 0.0, 0.0], 0.3), nodes=[2, 5])], seed=1)
    graphs.append(tc.Graph(base, one.frames, None))                                          # a fixed frame nothing uses
    graphs.append(tc.Graph(pc.Graph(base.submaps, base.nodes, base.constraints[:0]), one.frames, one.frame_constraints))
    graphs.append(tc.Graph(pc.Graph(base.submaps, base.nodes, base.constraints, np.ones(3, np.uint8), np.ones(12, np.uint8)),
                           one.frames, one.frame_constraints))                               # everything else constant
    graphs.append(tc.Graph(pc.Graph(base.submaps[:0], base.nodes, base.constraints[:0], gravity=-1), one.frames,
                           np.concatenate([one.frame_constraints, one.frame_constraints])))  # no submap, duplicates
    paths = []
    for i, g in enumerate(graphs):
        paths.append(str(tmp_path / ("graph%d.bin" % i)))
        pc._write(g, paths[-1], 0, 0, 1e4)
    out = subprocess.check_output([check] + paths).decode().splitlines()
    print("\n".join(out))
    assert len(out) == len(graphs) and all(" ok columns " in line for line in out)
    columns = [pc.structure_check_fields(line)["columns"] for line in out]
    assert columns[-4:] == [2 + 6 * 2, 4, 4, 4]
    assert columns[len(tc.CASES) + len(pc.CASES) + 3:][:4] == [256, 260, 256, 260]
    for key, index, value in (("submap", 1, 1), ("submap", 0, -1), ("node", 1, 12)):
        bad = tc.Graph(base, one.frames, one.frame_constraints.copy())
        bad.frame_constraints[key][index] = value
        pc._write(bad, paths[0], 0, 0, 1e4)
        assert subprocess.check_output([check, paths[0]]).decode().split()[-2:] == ["status", "1"]


def test_the_adapter_still_refuses_landmarks(tmp_path):
    """OptimizationProblem3D::Solve with a non-empty landmark_nodes ends in Check's abort (the reference's CHECK), before a
    context is touched: tests/cpp/pose_graph_terms_adapter.cc --landmark, on a problem without a context."""
    import __graft_entry__
    dl = __graft_entry__.build()
    exe = str(tmp_path / "pose_graph_terms_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "pose_graph_terms_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    done = subprocess.run([exe, "--landmark"], stderr=subprocess.PIPE)
    assert done.returncode == -6 and b"landmarks are not supported" in done.stderr
