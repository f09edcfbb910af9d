"""ICP without a GPU: the CPU model of tests/icp_common.py against independent references (scipy's kd-tree, math.fsum,
numpy's SVD), its convergence rules on constructed sequences, and the new names, struct layouts and adapter."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_common as ic  # noqa: E402


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


# ---- the search ----------------------------------------------------------------------------------------------------------------
def test_model_search_equals_kd_tree():
    """The float32 brute-force model against cKDTree (double arithmetic) on 3000 x 4000 scan-like points: the same
    neighbour wherever the two nearest double distances differ by more than float rounding can bridge (d2's three
    roundings and the coordinates' differences: 1e-5 relative is generous), and then d2 equal to 1e-6 relative."""
    rng = np.random.RandomState(1)
    t = rng.uniform(-30, 30, (4000, 3)).astype(np.float32)
    t[:2000, 2] = -1.8
    q = (t[rng.randint(0, 4000, 3000)] + rng.normal(0, 0.3, (3000, 3))).astype(np.float32)
    j, d2 = ic.nn_search(q, t)
    dist, k = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=2)
    clear = dist[:, 1] - dist[:, 0] > 1e-5 * dist[:, 1]
    print("clear of a tie:", int(clear.sum()), "of", len(q))
    assert clear.sum() > 2900
    assert np.array_equal(j[clear], k[clear, 0])
    assert np.allclose(d2[clear], dist[clear, 0] ** 2, rtol=1e-6, atol=1e-12)
    # within the bound: the same neighbours while they are within D, none beyond
    jb, d2b = ic.nn_search(q, t, 0.4)
    inside = d2.astype(np.float64) <= 0.4 * 0.4
    assert np.array_equal(jb[inside], j[inside]) and (jb[~inside] == -1).all() and np.isinf(d2b[~inside]).all()
    assert 100 < inside.sum() < 2900


def test_model_lattice_ties_go_to_the_lowest_index():
    g = np.arange(4, dtype=np.float32)
    targets = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    centres = targets[(targets < 3).all(axis=1)] + np.float32(0.5)
    j, d2 = ic.nn_search(centres, targets)
    assert (d2 == 0.75).all()  # eight corners at the same distance
    i = (centres - 0.5).astype(np.int64)
    assert np.array_equal(j, (i[:, 0] * 4 + i[:, 1]) * 4 + i[:, 2])
    order = np.random.RandomState(0).permutation(64)  # the index decides, not the position
    j2, _ = ic.nn_search(centres, targets[order])
    for row, c in enumerate(centres):
        corners = np.flatnonzero((np.abs(targets[order] - c) == 0.5).all(axis=1))
        assert len(corners) == 8 and j2[row] == corners.min()


def test_model_ignores_non_finite_points():
    t = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 1, 1]])
    q = np.float32([[0.9, 0, 0], [np.nan, 0, 0], [5, 5, np.inf], [0.1, 0, 0]])
    j, d2 = ic.nn_search(q, t)
    assert list(j) == [2, -1, -1, 0] and np.isinf(d2[1]) and np.isinf(d2[2])
    assert list(ic.nn_search(q, np.full((3, 3), np.nan, np.float32))[0]) == [-1] * 4
    far = np.float32([[3e38, 0, 0], [-3e38, 0, 0]])  # every d2 overflows: still the lowest index, kept without a bound
    j, d2 = ic.nn_search(np.float32([[0, 3e38, 0]]), far)
    assert j[0] == 0 and np.isinf(d2[0])


# ---- the tree ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 877, 2048, 2049, 5000, 70000])
def test_tree_sum_against_fsum(n):
    """A pairwise tree of depth L = log2(leaves) errs by at most L u sum|x| to first order, u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2: gamma_L = L u / (1 - L u)); math.fsum is the correctly rounded sum, within
    u |sum| of the real one.  Bound: gamma_L sum|x| + u |sum|."""
    rng = np.random.RandomState(n)
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 4, n)
    got = float(ic.tree_sum(x)[0])
    exact = math.fsum(x)
    leaves = max(ic.TREE_MIN_LEAVES, 1 << (n - 1).bit_length())
    depth = leaves.bit_length() - 1
    u = 2.0 ** -53
    bound = depth * u / (1 - depth * u) * math.fsum(np.abs(x)) + u * abs(exact)
    print("n", n, "depth", depth, "error", abs(got - exact), "bound", bound)
    assert abs(got - exact) <= bound
    # the order is a function of the index alone: zeros appended, or another shape, change no bit
    assert float(ic.tree_sum(np.concatenate([x, np.zeros(17)]))[0]) == got or leaves < n + 17
    two = ic.tree_sum(np.stack([x, -x], axis=1))
    assert two[0] == got and two[1] == -got


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def solve_pairs(kind, seed, n=400):
    rng = np.random.RandomState(seed)
    p = rng.uniform(-50, 50, (n, 3))
    if kind == "planar":
        p[:, 2] = 3.0
    if kind == "nearly_planar":
        p[:, 2] = 3.0 + 1e-4 * rng.standard_normal(n)
    if kind == "nearly_collinear":
        d = rng.standard_normal(3)
        p = np.outer(rng.uniform(-50, 50, n), d / np.linalg.norm(d)) + 1e-2 * rng.standard_normal((n, 3)) + rng.uniform(-20, 20, 3)
    p = p.astype(np.float32)
    motion = ic.synth.perturb_pose(ic.IDENTITY7, 2.0, 30.0, seed=seed + 100)
    q = (ic.synth.transform_points(motion, p).astype(np.float64) + 1e-3 * rng.standard_normal((n, 3))).astype(np.float32)
    return p, q


# Worst |R - R_svd| and |t - t_svd| (any entry) over the 20 seeds of each kind, measured once (x86-64, numpy 2
# on OpenBLAS): the assertion is ten times that.  A line of points with 1 cm of scatter over 100 m leaves
# the turn about the line determined only to the scatter's 1e-4 share: a condition number near 1e8, and both solves are
# 3e-8 apart there, each as good as the other.
MEASURED_SOLVE_DISAGREEMENT = {"random": 1.9e-15, "planar": 2.0e-15, "nearly_planar": 1.8e-15, "nearly_collinear": 3.4e-8}


@pytest.mark.parametrize("kind", list(MEASURED_SOLVE_DISAGREEMENT))
def test_solve_against_svd_kabsch(kind):
    worst = 0.0
    for seed in range(20):
        p, q = solve_pairs(kind, seed)
        sums, n = ic.correspondence_sums(p, q, np.arange(len(p), dtype=np.int32), np.zeros(len(p), np.float32))
        R, t = ic.solve(sums, n)
        R, t = np.array(R), np.array(t)
        Rk, tk = ic.kabsch(p.astype(np.float64), q.astype(np.float64))
        assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(R.T @ R - np.eye(3)).max() < 1e-14  # a proper rotation
        worst = max(worst, np.abs(R - Rk).max(), np.abs(t - tk).max())
    print(kind, "worst disagreement with the SVD", worst, "measured", MEASURED_SOLVE_DISAGREEMENT[kind])
    assert worst <= 10.0 * MEASURED_SOLVE_DISAGREEMENT[kind]


def test_solve_of_exact_pairs_and_of_a_line():
    p = np.float32([[0, 0, 0], [4, 0, 0], [0, 2, 0], [0, 0, 1], [3, 3, 3]])
    R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # a quarter turn about z: exact in floats
    q = (p @ R0.T + [1.0, 2.0, 3.0]).astype(np.float32)
    sums, n = ic.correspondence_sums(p, q, np.arange(5, dtype=np.int32), np.zeros(5, np.float32))
    R, t = ic.solve(sums, n)
    assert np.abs(np.array(R) - R0).max() < 1e-15 and np.abs(np.array(t) - [1.0, 2.0, 3.0]).max() < 1e-14
    # exactly collinear pairs (no rule of their own, dliom.h): still a proper rotation that maps the line onto the line
    line = np.outer(np.arange(6, dtype=np.float32), np.float32([1, 2, 2]))
    moved = (line @ R0.T).astype(np.float32)
    sums, n = ic.correspondence_sums(line, moved, np.arange(6, dtype=np.int32), np.zeros(6, np.float32))
    R, t = ic.solve(sums, n)
    R = np.array(R)
    assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(line @ R.T + t - moved).max() < 1e-13


# ---- the decisions ---------------------------------------------------------------------------------------------------------------
def turn_z(angle):
    c, s = math.cos(angle), math.sin(angle)
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


def test_convergence_rules_fire_in_order():
    o = ic.options()
    big = (turn_z(0.1), [0.5, 0.0, 0.0])  # far from the transformation thresholds
    # 1. the iteration count comes first, whatever else holds
    assert ic.decide(100, turn_z(0.0), [0.0] * 3, 1.0, 1.0, o) == ic.ITERATIONS
    assert ic.decide(1, *big, 5.0, ic.INF, ic.options(maximum_iterations=1)) == ic.ITERATIONS
    assert ic.decide(1, *big, 5.0, ic.INF, ic.options(maximum_iterations=0)) == ic.ITERATIONS  # 0 runs one iteration
    # 2. a small rotation AND a small translation: cos >= 1 - 1e-5 is |angle| <= 4.47e-3; t.t <= 1e-6 is |t| <= 1e-3
    assert ic.decide(2, turn_z(4.4e-3), [9.9e-4, 0.0, 0.0], 5.0, 9.0, o) == ic.TRANSFORM
    assert ic.decide(2, turn_z(4.6e-3), [0.0] * 3, 5.0, 9.0, o) == ic.NOT_CONVERGED
    assert ic.decide(2, turn_z(0.0), [1.1e-3, 0.0, 0.0], 5.0, 9.0, o) == ic.NOT_CONVERGED
    assert ic.decide(2, turn_z(0.0), [1e-3, 0.0, 0.0], 5.0, 9.0, ic.options(transformation_epsilon=1e-3 * 1e-3)) == ic.TRANSFORM  # inclusive
    # 3. the absolute change of the mean squared error, strict
    assert ic.decide(2, *big, 5.0, 5.0 + 5e-7, o) == ic.ABS_MSE
    assert ic.decide(2, *big, 5.0, 5.0, ic.options(euclidean_fitness_epsilon=0.0, relative_mse_epsilon=0.0)) == ic.NOT_CONVERGED
    # 4. the relative change: 4e-6 of 1e3 is not below 1e-6 absolutely, but 4e-9 relatively
    assert ic.decide(2, *big, 1e3, 1e3 + 4e-6, o) == ic.REL_MSE
    assert ic.decide(2, *big, 1e3, 1e3 + 2e-2, o) == ic.NOT_CONVERGED
    # the first iteration: |mse - inf| = inf fails 3, inf / inf = NaN fails 4 (IEEE: every comparison with NaN is false)
    assert ic.decide(1, *big, 5.0, ic.INF, o) == ic.NOT_CONVERGED
    assert ic.decide(1, *big, 5.0, ic.INF, ic.options(euclidean_fitness_epsilon=1e300, relative_mse_epsilon=1e300)) == ic.NOT_CONVERGED
    with np.errstate(all="ignore"):
        assert math.isnan(float(np.float64(ic.INF) / np.float64(ic.INF))) and not (float("nan") < 1e300)
    # 0 / 0 (two perfect iterations) is NaN as well, but 3 has fired before unless its epsilon is 0
    assert ic.decide(2, *big, 0.0, 0.0, o) == ic.ABS_MSE
    assert ic.decide(2, *big, 0.0, 0.0, ic.options(euclidean_fitness_epsilon=0.0)) == ic.NOT_CONVERGED


def test_model_alignments_end_as_constructed():
    source, target, motion = ic.moved_copy()
    assert (len(source), len(target)) == (877, 1753)
    r = ic.align(source, target)
    back = r["transform"] @ motion
    assert r["converged"] == 1 and r["reason"] == ic.TRANSFORM and 3 <= r["iterations"] <= 6
    assert np.linalg.norm(back[:3, 3]) < 1e-6 and np.abs(back[:3, :3] - np.eye(3)).max() < 1e-6
    r = ic.align(source, target, o=ic.options(maximum_iterations=1))
    assert (r["converged"], r["reason"], r["iterations"]) == (1, ic.ITERATIONS, 1)
    r = ic.align(source, target, o=ic.options(max_correspondence_distance=1e-4))
    assert (r["converged"], r["reason"], r["iterations"]) == (0, ic.NO_CORRESPONDENCES, 0) and r["correspondences"] < 3
    assert np.array_equal(r["transform"], np.eye(4)) and np.array_equal(r["aligned"], source)
    # a coarse absolute epsilon ends the loop on the mean squared error before the transformation is small
    r = ic.align(ic.ground_scan(0.35), ic.ground_scan(0.30), o=ic.options(euclidean_fitness_epsilon=0.5))
    assert r["reason"] == ic.ABS_MSE and r["iterations"] >= 2
    r = ic.align(ic.ground_scan(0.35), ic.ground_scan(0.30), o=ic.options(relative_mse_epsilon=0.5))
    assert r["reason"] == ic.REL_MSE and r["iterations"] >= 2


# ---- names, layouts, arguments, the adapter ------------------------------------------------------------------------------------
def test_constants_and_symbols(dl):
    header = open(os.path.join(ic.ROOT, "include", "dliom.h")).read()
    for name, value in (("NN_MAX_SHELLS", dl.NN_MAX_SHELLS), ("NN_MAX_CELLS_PER_AXIS", dl.NN_MAX_CELLS_PER_AXIS),
                        ("ICP_JACOBI_SWEEPS", ic.JACOBI_SWEEPS), ("ICP_TREE_MIN_LEAVES", ic.TREE_MIN_LEAVES)):
        assert int(re.search(r"#define DLIOM_%s (\d+)" % name, header).group(1)) == value
    assert dl.ICP_JACOBI_SWEEPS == ic.JACOBI_SWEEPS and dl.ICP_TREE_MIN_LEAVES == ic.TREE_MIN_LEAVES
    assert (dl.ICP_NOT_CONVERGED, dl.ICP_ITERATIONS, dl.ICP_TRANSFORM, dl.ICP_ABS_MSE, dl.ICP_REL_MSE, dl.ICP_NO_CORRESPONDENCES) == \
        (ic.NOT_CONVERGED, ic.ITERATIONS, ic.TRANSFORM, ic.ABS_MSE, ic.REL_MSE, ic.NO_CORRESPONDENCES)
    for name in ("DLIOM_ICP_NOT_CONVERGED = 0", "DLIOM_ICP_ITERATIONS = 1", "DLIOM_ICP_TRANSFORM = 2", "DLIOM_ICP_ABS_MSE = 3",
                 "DLIOM_ICP_REL_MSE = 4", "DLIOM_ICP_NO_CORRESPONDENCES = 5", "DLIOM_NN_AUTO = 0", "DLIOM_NN_BRUTE_FORCE = 1"):
        assert name in header
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_nn_index_create", "dliom_nn_index_destroy", "dliom_nn_index_memory_stats", "dliom_nn_index_query",
              "dliom_icp_default_options", "dliom_icp_align", "dliom_icp_step"):
        assert n in names and getattr(dl.load_library(), n) is not None
    assert "parity unpinned against pcl" in header.lower()


def test_default_options_and_presets(dl):
    o = dl.ground_truth_icp_options()
    assert (o.max_correspondence_distance, o.maximum_iterations, o.transformation_epsilon, o.euclidean_fitness_epsilon) == \
        (30.0, 100, 1e-6, 1e-6)
    assert (o.rotation_epsilon, o.relative_mse_epsilon, o.min_correspondences, o.search, o.reserved) == (1e-5, 1e-5, 3, dl.NN_AUTO, 0)
    m = dl.match_by_icp_options()
    assert m.max_correspondence_distance == 3.0 and m.maximum_iterations == 100
    for k, v in ic.DEFAULTS.items():
        assert getattr(o, k) == v


def test_argument_checks(dl):
    L = dl.load_library()
    h = C.c_void_p()
    assert L.dliom_nn_index_create(None, None, None, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_nn_index_memory_stats(None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_nn_index_query(None, None, None, 1.0, 0, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_icp_default_options(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_icp_align(None, None, None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_icp_step(None, None, None, None, None, None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    L.dliom_nn_index_destroy(None)  # like free()


def test_struct_layouts_match_header(dl, tmp_path):
    src = tmp_path / "sizes.c"
    names = ["dliom_nn_index_options", "dliom_nn_query_stats", "dliom_nn_index_memory", "dliom_icp_options", "dliom_icp_result"]
    offsets = [("dliom_icp_result", "transform"), ("dliom_icp_result", "fitness_count"), ("dliom_icp_result", "search_ms"),
               ("dliom_icp_options", "maximum_iterations"), ("dliom_nn_index_memory", "cell_edge")]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dliom.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * (len(names) + len(offsets))),
                    ", ".join(["sizeof(%s)" % n for n in names] + ["offsetof(%s, %s)" % o for o in offsets])))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    types = (dl.NnIndexOptions, dl.NnQueryStats, dl.NnIndexMemory, dl.IcpOptions, dl.IcpResult)
    assert got[:len(names)] == [C.sizeof(t) for t in types]
    assert got[len(names):] == [dl.IcpResult.transform.offset, dl.IcpResult.fitness_count.offset, dl.IcpResult.search_ms.offset,
                                dl.IcpOptions.maximum_iterations.offset, dl.NnIndexMemory.cell_edge.offset]


def test_adapter_known_answers(dl, tmp_path):
    """tests/cpp/icp_adapter_kat.cc builds with g++ -Wall -Werror (the IterativeClosestPoint adapter with it) and holds:
    FormatGroundTruthLine byte-equal to an ostream, FindRevisitNode on a hand-made trajectory."""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path / "icp_adapter_kat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "icp_adapter_kat.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "ok"
