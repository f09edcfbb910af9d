"""NDT without a GPU: the CPU model of tests/ndt_common.py against independent means (a numpy group-by with np.cov,
numpy's eigh and pinv, math.exp, scipy's kd-tree, central differences), the adapter's ApproximateVoxelGrid against a Python
model of its statement, and the new names, struct layouts and argument checks of the library."""
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
import ndt_common as nd  # noqa: E402


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def ground_cells():
    return nd.build_cells(ic.ground_scan())


GENERIC_P = [0.05, -0.03, 0.02, 0.01, -0.02, 0.015]


# ---- cells -----------------------------------------------------------------------------------------------------------------
def test_cells_equal_a_numpy_group_by(ground_cells):
    """Every cell of the ground scan against a plain group-by on float64 floor(x / 1.0): members, mean, and np.cov(ddof=1)
    against the covariance rebuilt from icov.  The header's C (PCL 1.8.0's) is the population covariance times (n - 1) / n,
    that is np.cov(ddof=1) times ((n - 1) / n)^2: the factor is applied to numpy's value here.  The one-pass moments lose
    about eps * |x|^2 / var = 2e-16 * 1e3 / 1e-3 of a covariance entry at the worst (30 m ranges, millimetre spreads): 1e-9 absolute is generous; icov's inverse is compared
    where the raised eigenvalue floor did not change it."""
    t = ic.ground_scan().astype(np.float64)
    groups = {}
    for i, c in enumerate(np.floor(t).astype(int)):
        groups.setdefault(tuple(c), []).append(i)
    cells = ground_cells
    assert len(cells["n"]) == len(groups) and cells["kept_points"] == len(t)
    order = sorted(groups, key=lambda c: (c[2], c[1], c[0]))
    assert [tuple(c) for c in cells["index"]] == order
    checked = 0
    for k, c in enumerate(order):
        x = t[groups[c]]
        assert cells["n"][k] == len(x)
        assert np.allclose(cells["mean"][k], x.mean(axis=0), rtol=0, atol=1e-12)
        if len(x) < 6:
            assert not cells["valid"][k]
            continue
        cov = np.cov(x.T, ddof=1) * ((len(x) - 1.0) / len(x)) ** 2
        lam = np.linalg.eigvalsh(cov)
        if cells["valid"][k] and lam[0] > 0.011 * lam[2]:
            icov = nd.full_icov(cells["icov"][k:k + 1])[0]
            assert np.allclose(np.linalg.inv(icov), cov, rtol=1e-6, atol=1e-9)
            checked += 1
    print("valid cells:", int(cells["valid"].sum()), "compared with np.cov:", checked)
    assert cells["valid"].sum() >= 20 and checked >= 3


def test_cell_rules():
    """n below the minimum, identical points and a flat cell; the eigenvalue floor"""
    rng = np.random.RandomState(2)
    five = rng.uniform(0.1, 0.9, (5, 3))
    same = np.tile([[1.5, 0.5, 0.5]], (8, 1))
    flat = np.c_[rng.uniform(2.1, 2.9, (9, 2)), np.full(9, 0.5)]
    cells = nd.build_cells(np.r_[five, same, flat].astype(np.float32))
    assert list(cells["n"]) == [5, 8, 9] and list(cells["valid"]) == [False, False, True]
    icov = nd.full_icov(cells["icov"][2:3])[0]
    lam = np.linalg.eigvalsh(np.linalg.inv(icov))
    assert abs(lam[0] / lam[2] - 0.01) < 1e-9  # the flat direction is raised to a hundredth of the largest


def test_pow2_tree_is_the_stated_tree():
    v = np.random.RandomState(3).uniform(-1, 1, (5, 2))
    want = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + 0.0) + (0.0 + 0.0))
    assert np.array_equal(nd.pow2_tree_sum(v), want)
    assert np.array_equal(nd.pow2_tree_sum(v[:1]), v[0])


# ---- eigen -----------------------------------------------------------------------------------------------------------------
def test_jacobi_equals_eigh_and_pinv():
    """3x3: eigenvalues to 1e-12 of the largest, eigenvectors to 1e-9 up to sign (gaps of the random matrices are > 1e-3).
    6x6 pseudo-inverse to 1e-9 relative on a well-conditioned matrix, and on a rank-4 one (the dropped eigenvalues are 1e-16
    of the largest, below the header's 6 * 2^-52)."""
    rng = np.random.RandomState(4)
    for _ in range(50):
        a = rng.normal(size=(3, 3))
        Cm = a @ a.T
        lam, V, order = nd.eigen3(Cm)
        w, U = np.linalg.eigh(Cm)
        assert np.allclose(lam, w, rtol=0, atol=1e-12 * w[2])
        V = np.array(V)[:, order]
        for k in range(3):
            assert min(np.abs(V[:, k] - U[:, k]).max(), np.abs(V[:, k] + U[:, k]).max()) < 1e-9
    for rank in (6, 4):
        a = rng.normal(size=(6, rank))
        Hm = a @ a.T
        got, want = nd.pinv6(Hm), np.linalg.pinv(Hm, rcond=1e-12)
        print("rank", rank, "pinv difference", np.abs(got - want).max() / np.abs(want).max())
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
        g = rng.normal(size=6)
        assert np.allclose(nd.newton_step(Hm, g), -want @ g, rtol=1e-8, atol=1e-9 * np.abs(want @ g).max())


# ---- E -----------------------------------------------------------------------------------------------------------------------
def test_exponential_within_two_ulp():
    u = np.concatenate([np.random.RandomState(5).uniform(-708.0, 0.0, 100000), [0.0, -0.0, -708.0]])
    got = nd.E(u)
    want = np.array([math.exp(v) for v in u])
    ulp = np.abs(got - want) / np.spacing(want)
    print("worst:", ulp.max(), "ulp")
    assert ulp.max() <= 2.0
    assert nd.E(np.array([0.0]))[0] == 1.0 and nd.E(np.array([-708.1]))[0] == 0.0 and np.isnan(nd.E(np.array([np.nan]))[0])


# ---- neighbours ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_neighbours_equal_kd_tree_ball(ground_cells, seed):
    """The 27-cell rule against cKDTree.query_ball_point (double) on the valid cells' centroids, every query, none left
    out.  The two can differ only where a distance is within float rounding of the radius; for these seeds no query of the
    400 is (checked on this CPU: all five seeds agree everywhere)."""
    rng = np.random.default_rng(seed)
    t = ic.ground_scan()
    q = (t[rng.integers(0, len(t), 400)] + rng.normal(0, 0.4, (400, 3))).astype(np.float32)
    got = [set() for _ in q]
    for qi, ci in nd.neighbours(ground_cells, q, 1.0):
        for a, b in zip(qi, ci):
            got[a].add(int(b))
    want = cKDTree(ground_cells["valid_mean"]).query_ball_point(q.astype(np.float64), 1.0)
    assert sum(1 for g in got if g) > 50
    assert all(g == set(w) for g, w in zip(got, want))


def test_neighbour_order_and_inclusive_radius():
    """One valid cell; queries at exactly r (kept), an ulp beyond (dropped), and in the 26 cells around it"""
    rng = np.random.RandomState(6)
    cell = (np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (16, 3))).astype(np.float32)
    cells = nd.build_cells(cell)
    assert list(cells["valid"]) == [True]
    m = cells["valid_mean"][0].astype(np.float32)
    at_r = np.array([m[0] + np.float32(1.0), m[1], m[2]], np.float32)
    dx = at_r[0] - m[0]
    assert dx * dx <= np.float32(1.0)  # (otherwise the construction below needs another seed)
    beyond = at_r.copy()
    beyond[0] = np.nextafter(np.nextafter(at_r[0], np.float32(9)), np.float32(9))
    assert (beyond[0] - m[0]) ** 2 > np.float32(1.0)
    pairs = nd.neighbours(cells, np.array([at_r, beyond, m]), 1.0)
    found = sorted(int(a) for qi, _ in pairs for a in qi)
    assert found == [0, 2]
    # the query in the cell's own index sees it at offset (0,0,0), the 14th of the order; one at +x sees it at (-1,0,0)
    assert list(pairs[13][0]) == [2] and list(pairs[12][0]) == [0]


# ---- derivatives -----------------------------------------------------------------------------------------------------------
def test_point_derivatives_against_central_differences():
    """J and H of R(a, b, c) x against central differences (h = 1e-5, |x| <= 35 m).  Measured on this CPU: 7.0e-10 for both
    (h^2 |x| / 6 truncation plus eps |x| / h rounding); asserted: ten times that."""
    rng = np.random.default_rng(1)
    x = rng.uniform(-20, 20, (50, 3)).astype(np.float32).astype(np.float64)
    ang = [0.3, -0.7, 1.1]

    def Rx(a, b, c):
        return x @ np.array(nd.pose_terms([0, 0, 0, a, b, c])[0]).T

    def Jcol(j):
        return lambda a, b, c: nd.point_vectors(x, nd.pose_terms([0, 0, 0, a, b, c])[2], 3)[:, j]

    def central(f, i, h=1e-5):
        up, down = list(ang), list(ang)
        up[i] += h
        down[i] -= h
        return (f(*up) - f(*down)) / (2 * h)

    _, _, J, H = nd.pose_terms([0, 0, 0] + ang)
    Jv, Hv = nd.point_vectors(x, J, 3), nd.point_vectors(x, H, 6)
    worst_j = max(np.abs(central(Rx, i) - Jv[:, i]).max() for i in range(3))
    worst_h = max(np.abs(central(Jcol(j), i) - Hv[:, nd.HESSIAN_OF[(3 + i, 3 + j)]]).max() for i in range(3) for j in range(i, 3))
    print("J:", worst_j, "H:", worst_h)
    assert worst_j <= 7.0e-9 and worst_h <= 7.0e-9  # measured 7.0e-10, 7.0e-10


def test_score_derivatives_against_central_differences(ground_cells):
    """The gradient against central differences of the score, the Hessian against those of the gradient, on the moved copy
    at a generic p with h = 1e-4.  The score is only piecewise smooth (x' is rounded to float, neighbours come and go), so
    the differences carry that noise.  Measured on this CPU, relative to the largest entry: 1.43e-4 (gradient), 1.41e-4
    (Hessian); asserted: ten times that.  A wrong sign or a missing term shows as O(1)."""
    source = ic.moved_copy()[0]
    e = nd.evaluate(ground_cells, source, GENERIC_P)
    g, Hn = np.zeros(6), np.zeros((6, 6))
    h = 1e-4
    for i in range(6):
        up, down = list(GENERIC_P), list(GENERIC_P)
        up[i] += h
        down[i] -= h
        a, b = (nd.evaluate(ground_cells, source, p, what=nd.EVAL_GRADIENT) for p in (up, down))
        g[i] = (a["score"] - b["score"]) / (2 * h)
        Hn[i] = (a["gradient"] - b["gradient"]) / (2 * h)
    rel_g = np.abs(g - e["gradient"]).max() / np.abs(e["gradient"]).max()
    rel_h = np.abs(Hn - e["hessian"]).max() / np.abs(e["hessian"]).max()
    print("gradient:", rel_g, "hessian:", rel_h)
    assert rel_g <= 1.43e-3 and rel_h <= 1.41e-3  # measured 1.43e-4, 1.41e-4
    assert np.array_equal(e["hessian"], e["hessian"].T) and e["pairs"] > 100


def test_evaluation_parts_have_the_same_bits(ground_cells):
    source = ic.moved_copy()[0]
    full = nd.evaluate(ground_cells, source, GENERIC_P)
    grad = nd.evaluate(ground_cells, source, GENERIC_P, what=nd.EVAL_GRADIENT)
    hess = nd.evaluate(ground_cells, source, GENERIC_P, what=nd.EVAL_HESSIAN)
    assert grad["score"] == full["score"] and np.array_equal(grad["gradient"], full["gradient"])
    assert np.array_equal(hess["hessian"], full["hessian"]) and not grad["hessian"].any() and not hess["gradient"].any()


# ---- pose ------------------------------------------------------------------------------------------------------------------
def test_angle_triple_rebuilds_its_rotation():
    rng = np.random.RandomState(7)
    for _ in range(200):
        p = [0.0, 0.0, 0.0] + list(rng.uniform(-math.pi, math.pi, 3))
        T = nd.transform_of(p)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
        back = nd.transform_of(nd.pose_of_guess(T))
        assert np.allclose(back, T, rtol=0, atol=1e-14)
    T = np.eye(4)
    T[:3, 3] = [1.0, -2.0, 3.0]
    assert nd.pose_of_guess(T) == [1.0, -2.0, 3.0, 0.0, 0.0, 0.0]
    d1, d2 = nd.constants(nd.options())
    assert d1 < 0.0 < d2


# ---- the adapter's filter ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adapter_kat(tmp_path_factory):
    """tests/cpp/ndt_adapter_kat.cc builds with g++ -Wall -Werror (the NDT adapter with it)"""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path_factory.mktemp("ndt") / "ndt_adapter_kat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"),
                           "-I", os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "ndt_adapter_kat.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    return exe


def test_adapter_known_answers(dl, adapter_kat):
    out = subprocess.run([adapter_kat], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip() == "ok"


@pytest.mark.parametrize("case", ["evicting", "quiet"])
def test_adapter_filter_equals_its_statement(dl, adapter_kat, tmp_path, case):
    """evicting: the ground scan at 1 m, 998 voxels through 512 slots: voxels gather points, are evicted and come back.
    quiet: 300 points in a 0.6 m cube at 0.2 m, 27 voxels whose slots are checked to be distinct: nothing is flushed before
    the end."""
    if case == "evicting":
        points, leaf = np.array(ic.ground_scan(), np.float32), 1.0
    else:
        points, leaf = np.random.RandomState(8).uniform(0.0, 0.6, (300, 3)).astype(np.float32), 0.2
        v = np.unique(np.floor(points * (np.float32(1) / np.float32(leaf))).astype(int), axis=0)
        assert len({int(a * 7171 + b * 3079 + c * 4231) & 511 for a, b, c in v}) == len(v)
    want = nd.approximate_voxel_grid(points, leaf)
    (tmp_path / "in.bin").write_bytes(points.tobytes())
    subprocess.check_call([adapter_kat, "filter", repr(leaf), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(-1, 3)
    print(case, len(points), "->", len(got))
    assert got.tobytes() == want.tobytes()
    assert (998 < len(got) < len(points)) if case == "evicting" else (len(got) == len(v) == 27)


# ---- motion recovery -------------------------------------------------------------------------------------------------------
def test_alignment_reduces_the_pose_error(ground_cells):
    """The moved copy (0.18 m, 1.5 degrees) from the identity, tool settings.  Measured on the model on this CPU: the
    translation error falls from 0.1796 m to 0.0710 m (a factor 2.53) under the clamped step and to 0.1172 m (1.53)
    under More-Thuente; asserted: half of each factor."""
    source, target, motion = ic.moved_copy()
    start = np.linalg.norm(motion[:3, 3])
    for mode, factor in ((nd.STEP_CLAMPED, 2.53), (nd.STEP_MORE_THUENTE, 1.53)):
        r = nd.align(ground_cells, source, target, None, nd.options(step_mode=mode))
        left = np.linalg.norm((r["transform"] @ motion)[:3, 3])
        print("mode", mode, "reason", r["reason"], "iterations", r["iterations"], "error", start, "->", left, "factor", start / left)
        assert r["converged"] == 1 and start / left >= factor / 2
        assert (r["evaluations_without_hessian"] > 0) == (mode == nd.STEP_MORE_THUENTE)
        assert r["fitness_count"] == len(source) and r["fitness_score"] > 0.0


def test_model_alignment_ends():
    """No valid cell: all zeros, DLIOM_NDT_ZERO_STEP at once.  maximum_iterations 0 and 1: two and three passes."""
    source, target, _ = ic.moved_copy()
    empty = nd.build_cells(target[:5])
    r = nd.align(empty, source)
    assert (r["converged"], r["reason"], r["iterations"], r["score"], r["pairs"]) == (1, nd.ZERO_STEP, 0, 0.0, 0)
    cells = nd.build_cells(target)
    for most, passes in ((0, 2), (1, 3)):
        r = nd.align(cells, source[::4], o=nd.options(maximum_iterations=most, transformation_epsilon=0.0))
        assert (r["converged"], r["reason"], r["iterations"]) == (1, nd.ITERATIONS, passes)
        assert r["evaluations_with_hessian"] == passes + 1


# ---- the library without a device -----------------------------------------------------------------------------------------
def test_constants_and_symbols(dl):
    header = open(os.path.join(ic.ROOT, "include", "dliom.h")).read()
    for name, value in (("NDT_JACOBI_SWEEPS", nd.JACOBI_SWEEPS), ("NDT_PINV_SWEEPS", nd.PINV_SWEEPS)):
        assert int(re.search(r"#define DLIOM_%s (\d+)" % name, header).group(1)) == value == getattr(dl, name)
    assert "#define DLIOM_NDT_MAX_CELL_INDEX (1 << 20)" in header and dl.NDT_MAX_CELL_INDEX == nd.HALF == 1 << 20
    for text in ("DLIOM_NDT_STEP_CLAMPED = 0, DLIOM_NDT_STEP_MORE_THUENTE = 1",
                 "DLIOM_NDT_NOT_CONVERGED = 0, DLIOM_NDT_ITERATIONS = 1, DLIOM_NDT_EPSILON = 2, DLIOM_NDT_ZERO_STEP = 3",
                 "DLIOM_NDT_EVAL_GRADIENT = 0, DLIOM_NDT_EVAL_ALL = 1, DLIOM_NDT_EVAL_HESSIAN = 2"):
        assert text in header
    assert (dl.NDT_STEP_CLAMPED, dl.NDT_STEP_MORE_THUENTE) == (nd.STEP_CLAMPED, nd.STEP_MORE_THUENTE)
    assert (dl.NDT_NOT_CONVERGED, dl.NDT_ITERATIONS, dl.NDT_EPSILON, dl.NDT_ZERO_STEP) == \
        (nd.NOT_CONVERGED, nd.ITERATIONS, nd.EPSILON, nd.ZERO_STEP)
    assert (dl.NDT_EVAL_GRADIENT, dl.NDT_EVAL_ALL, dl.NDT_EVAL_HESSIAN) == (nd.EVAL_GRADIENT, nd.EVAL_ALL, nd.EVAL_HESSIAN)
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_ndt_default_options", "dliom_ndt_target_create", "dliom_ndt_target_destroy", "dliom_ndt_target_memory_stats",
              "dliom_ndt_target_cells", "dliom_ndt_evaluate", "dliom_ndt_align"):
        assert n in names and getattr(dl.load_library(), n) is not None
    assert "scan alignment by ndt" in header.lower()


def test_default_options(dl):
    o = dl.ndt_options()
    for k, v in nd.DEFAULTS.items():
        assert getattr(o, k) == v
    assert o.reserved == 0
    with pytest.raises(TypeError):
        dl.ndt_options(no_such_option=1)


def test_argument_checks_before_the_device(dl):
    L = dl.load_library()
    h = C.c_void_p()
    o = dl.ndt_options()
    assert L.dliom_ndt_default_options(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_target_create(None, None, C.byref(o), C.byref(h)) == dl.ERR_INVALID_ARGUMENT and not h.value
    assert L.dliom_ndt_target_memory_stats(None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_target_cells(None, None, 0, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_evaluate(None, None, None, C.byref(o), 1, None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_align(None, None, None, C.byref(o), None, None, None) == dl.ERR_INVALID_ARGUMENT
    L.dliom_ndt_target_destroy(None)  # like free()


def test_struct_layouts_match_header(dl, tmp_path):
    src = tmp_path / "sizes.c"
    names = ["dliom_ndt_options", "dliom_ndt_cell", "dliom_ndt_target_memory", "dliom_ndt_result"]
    offsets = [("dliom_ndt_options", "maximum_iterations"), ("dliom_ndt_options", "step_mode"), ("dliom_ndt_cell", "n"),
               ("dliom_ndt_cell", "icov"), ("dliom_ndt_target_memory", "build_ms"), ("dliom_ndt_result", "p"),
               ("dliom_ndt_result", "transform"), ("dliom_ndt_result", "fitness_count"), ("dliom_ndt_result", "evaluate_ms")]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dliom.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * (len(names) + len(offsets))),
                    ", ".join(["sizeof(%s)" % n for n in names] + ["offsetof(%s, %s)" % o for o in offsets])))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    types = {"dliom_ndt_options": dl.NdtOptions, "dliom_ndt_cell": dl.NdtCell, "dliom_ndt_target_memory": dl.NdtTargetMemory,
             "dliom_ndt_result": dl.NdtResult}
    assert got[:len(names)] == [C.sizeof(types[n]) for n in names]
    assert got[len(names):] == [getattr(types[s], f).offset for s, f in offsets]
