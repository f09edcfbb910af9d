"""The pose graph solve without a GPU: the CPU model (tests/cpp/pose_graph_model.cc) against the reference's own test,
against hand computations and against an independent minimiser; the honesty of the parity cases; and the host structure
builder (d-liom_amd/csrc/pose_graph_structure.h) under sanitisers, as a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import least_squares

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
from pose_graph_common import synth  # noqa: E402


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_graph_model")
    return pc.build_model(d), d


def numpy_residual(submap, node, zbar, tw, rw):
    """e of cost_helpers_impl.h:57-101 written independently: rotation matrices and an arccos-free angle-axis."""
    def matrix(q):
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    e_t = zbar[:3] - matrix(submap[3:]).T @ (node[:3] - submap[:3])
    q = synth._quat_mul(synth._quat_mul(node[3:] * [1, -1, -1, -1], submap[3:]), zbar[3:])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    n = np.linalg.norm(q[1:])
    angle = 2 * np.arctan2(n, q[0])
    e_r = q[1:] * (angle / n if n > 1e-12 else 2.0)
    return np.concatenate([tw * e_t, rw * e_r])


def test_reference_reduces_noise(model):
    """optimization_problem_3d_test.cc:106-191 on the model, with either linear solver."""
    exe, d = model
    g, truth = pc.reduces_noise(exe, d)
    assert (len(g.submaps), len(g.nodes), len(g.constraints)) == (3, 100, 300)
    before = pc.noise_errors(truth, g.nodes)
    for solver in (pc.QR, pc.ELIMINATED):
        r = pc.model_solve(exe, g, d, solver)
        after = pc.noise_errors(truth, r["nodes"])
        print("solver", solver, "ratios", after[0] / before[0], after[1] / before[1], r["termination"], r["iterations"])
        assert 0.8 * before[0] > after[0] and 0.8 * before[1] > after[1]


@pytest.mark.parametrize("fix_z", [False, True])
def test_spot_checks(model, fix_z):
    exe, d = model
    g = pc.branches_graph(fix_z)
    cost, r, gradient, columns = pc.model_evaluate(exe, g, d)
    assert columns == (2 + 8 * 5 + 6 * 5 if fix_z else 2 + 8 * 6 + 6 * 6)
    # every residual against the hand-written one; the zero residual; the w < 0 flip near pi
    for c, k in enumerate(g.constraints):
        want = numpy_residual(g.submaps[k["submap"]], g.nodes[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"])
        assert np.allclose(r[c], want, rtol=1e-9, atol=1e-9), (c, r[c], want)
    assert np.abs(r[0]).max() < 1e-12
    for c in (2, 3):
        angle = np.linalg.norm(r[c, 3:]) / g.constraints[c]["rotation_weight"]
        assert 2.9 < angle <= np.pi, angle
    assert abs(cost - 0.5 * (r ** 2).sum()) <= 1e-12 * cost
    step = pc.model_step(exe, g, d, pc.QR)
    assert np.all(np.isfinite(step["blocks"]["js"])) and np.all(np.isfinite(step["blocks"]["jn"]))  # the angle < 1e-7 branch
    assert 0 in step["blocks"]["c"] and 14 not in step["blocks"]["c"]  # the fixed constraint has left
    # the gradient against central differences of the hand-written cost along the first submap's two rotation slots
    def total(submaps):
        return 0.5 * sum((numpy_residual(submaps[k["submap"]], g.nodes[k["node"]], k["zbar"], k["translation_weight"],
                                         k["rotation_weight"]) ** 2).sum() for k in g.constraints)
    for slot in (0, 1):
        h = 1e-6
        costs = []
        for sign in (1, -1):
            s = g.submaps.copy()
            v = np.zeros(3)
            v[slot] = sign * h
            s[0, 3:] = synth._quat_mul(s[0, 3:], np.concatenate([[1.0], v]))  # x (x) [1, d0, d1, 0]
            costs.append(total(s))
        assert abs((costs[0] - costs[1]) / (2 * h) - gradient[0, 3 + slot]) <= 1e-5 * max(1.0, abs(gradient[0, 3 + slot]))
    assert np.all(gradient[0, :3] == 0) and gradient[0, 5] == 0  # first submap: translation constant, two rotation columns
    assert np.all(gradient[9] == 0) and np.all(gradient[11 + 4] == 0) and np.all(gradient[10] == 0) and np.all(gradient[11 + 7] == 0)
    # a solve moves neither the first submap's translation, nor a constant block, nor (fix_z) any z
    solved = pc.model_solve(exe, g.with_options(max_iterations=50), d)
    assert solved["final_cost"] < solved["initial_cost"]
    assert solved["submaps"][0, :3].tobytes() == g.submaps[0, :3].tobytes()
    assert solved["submaps"][0, 3:].tobytes() != g.submaps[0, 3:].tobytes()
    assert solved["submaps"][9].tobytes() == g.submaps[9].tobytes() and solved["nodes"][4].tobytes() == g.nodes[4].tobytes()
    assert solved["submaps"][10].tobytes() == g.submaps[10].tobytes() and solved["nodes"][7].tobytes() == g.nodes[7].tobytes()
    # ConstantYawQuaternionPlus: one step turns the first submap about an axis in its own xy plane
    assert step["delta"][0, 5] == 0 and np.all(step["delta"][0, :3] == 0) and np.any(step["delta"][0, 3:5] != 0)
    if fix_z:
        assert solved["submaps"][:, 2].tobytes() == g.submaps[:, 2].tobytes()
        assert solved["nodes"][:, 2].tobytes() == g.nodes[:, 2].tobytes()
        assert np.all(step["delta"][:, 2] == 0)
    else:
        assert np.any(solved["nodes"][:, 2] != g.nodes[:, 2])


def test_independent_minimum(model):
    """The model's final cost against scipy.optimize.least_squares on the same residuals (written independently above),
    as tests/test_oracle_lm_independent.py does for the scan matcher: Ceres stops early (function tolerance 1e-6), so the
    model may not undercut the converged minimum and lies within 1e-4 of it."""
    exe, d = model
    g = pc.synthetic(4, 24, 1, seed=11, max_iterations=200)
    got = pc.model_solve(exe, g, d)
    S, N = len(g.submaps), len(g.nodes)

    def poses(p):
        s, n = g.submaps.copy(), g.nodes.copy()
        s[0, 3:] = synth._quat_mul(s[0, 3:], synth._quat_of([p[0], p[1], 0.0]))
        at = 2
        for arr, first in ((s, 1), (n, 0)):
            for i in range(first, len(arr)):
                arr[i, :3] += p[at:at + 3]
                arr[i, 3:] = synth._quat_mul(synth._quat_of(p[at + 3:at + 6]), arr[i, 3:])
                at += 6
        return s, n

    def fun(p):
        s, n = poses(p)
        return np.concatenate([numpy_residual(s[k["submap"]], n[k["node"]], k["zbar"], k["translation_weight"], k["rotation_weight"])
                               for k in g.constraints])
    sol = least_squares(fun, np.zeros(2 + 6 * (S - 1) + 6 * N), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
    cost_min = 0.5 * (sol.fun ** 2).sum()
    print("model", got["final_cost"], "scipy", cost_min, got["iterations"])
    assert got["columns"] == len(sol.x)
    assert got["final_cost"] >= cost_min * (1.0 - 1e-9)
    assert got["final_cost"] <= cost_min * (1.0 + 1e-4)
    assert got["initial_cost"] > 10 * got["final_cost"]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_parity_cases_are_honest(model, name):
    """Every case of the fixed list decides nothing on a knife's edge: no step quality within 1e-6 (relative) of
    min_relative_decrease, no tolerance test within 1e-6 of its threshold; and the model's linear solvers -- eliminated
    normal equations, which is the device's algorithm, and the Householder QR of [J; D], which forms no J^T J (with the
    structural zeros skipped on every case, and dense as LevenbergMarquardtStrategy has it where that is affordable) --
    give the same accept / reject sequence, iteration count and (to 1e-8) poses."""
    exe, d = model
    g = pc.CASES[name](exe, d)
    a = pc.model_solve(exe, g, d, pc.ELIMINATED)
    print(name, a["termination"], a["iterations"], a["steps"], a["rises"], a["quality_margin"], a["tolerance_margin"])
    assert a["quality_margin"] > 1e-6 and a["tolerance_margin"] > 1e-6
    assert a["termination"] in (0, 1) and a["successful"] >= 2 and 2 not in a["steps"]
    assert (0 in a["steps"]) == (name in pc.REJECTING) and (a["rises"] > 0) == (name in pc.RISING)
    for solver in (pc.SPARSE_QR,) + ((pc.QR,) if name in pc.QR_CASES else ()):
        b = pc.model_solve(exe, g, d, solver)
        assert b["quality_margin"] > 1e-6 and b["tolerance_margin"] > 1e-6
        assert (a["termination"], a["iterations"], a["steps"], a["rises"]) == (b["termination"], b["iterations"], b["steps"], b["rises"])
        assert np.abs(a["nodes"] - b["nodes"]).max() <= 1e-8 and np.abs(a["submaps"] - b["submaps"]).max() <= 1e-8


def test_structured_qr_is_the_dense_qr(model):
    """The structured QR step against LevenbergMarquardtStrategy's dense QR on the step cases that hold every branch."""
    exe, d = model
    for g in (pc.branches_graph(False), pc.branches_graph(True), pc.synthetic(7, 12, 1, seed=7)):
        a, b = pc.model_step(exe, g, d, pc.QR), pc.model_step(exe, g, d, pc.SPARSE_QR)
        assert np.abs(a["delta"] - b["delta"]).max() <= 1e-11 * np.abs(a["delta"]).max()
        assert np.array_equal(a["delta"] == 0, b["delta"] == 0)


def test_structure_builder_under_sanitizers(model, tmp_path):
    """tests/cpp/pose_graph_structure_check.cc, a stand-alone program built with -fsanitize=address,undefined, on the case
    list and on degenerate graphs."""
    exe, d = model
    check = pc.build_structure_check(tmp_path)
    graphs = [make(exe, d) for make in pc.CASES.values()] + [pc.branches_graph(False), pc.branches_graph(True)]
    base = pc.synthetic(3, 12, 0, seed=1)
    none = np.zeros(0, dtype=pc.CONSTRAINT)
    graphs.append(pc.Graph(base.submaps, base.nodes, none))                                  # no constraints
    graphs.append(pc.Graph(base.submaps[:0], base.nodes[:0], none, gravity=-1))              # nothing at all
    graphs.append(pc.Graph(base.submaps, base.nodes, base.constraints[base.constraints["node"] != 5]))    # a node with none
    graphs.append(pc.Graph(base.submaps, base.nodes, base.constraints[base.constraints["submap"] != 1]))  # a submap with none
    graphs.append(pc.Graph(base.submaps, base.nodes, np.concatenate([base.constraints, base.constraints, base.constraints[:3]])))
    graphs.append(pc.Graph(base.submaps, base.nodes, base.constraints, np.ones(3, np.uint8), np.ones(12, np.uint8)))  # all constant
    paths = []
    for i, g in enumerate(graphs):
        paths.append(str(tmp_path / ("graph%d.bin" % i)))
        pc._write(g, paths[-1], 0, 0, 1e4)
    out = subprocess.check_output([check] + paths).decode().splitlines()
    print("\n".join(out))
    assert len(out) == len(graphs) and all(" ok columns " in line for line in out)
    last = pc.structure_check_fields(out[-1])
    assert last["columns"] == 0 and last["kept"] == 0
    bad = pc.Graph(base.submaps, base.nodes, base.constraints.copy())
    bad.constraints["node"][4] = 12
    pc._write(bad, paths[0], 0, 0, 1e4)
    assert subprocess.check_output([check, paths[0]]).decode().split()[-2:] == ["status", "1"]
