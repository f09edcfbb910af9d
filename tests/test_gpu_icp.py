"""ICP and the exact nearest-neighbour index on the device against the CPU model of tests/icp_common.py: bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_common as ic  # noqa: E402

pytestmark = pytest.mark.gpu


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN standing for any other (a NaN's payload is not part of the statement)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def check_search(dl, ctx, targets, queries, max_distance=np.inf, cell_edge=0.0, modes=None):
    """The index's (j, d2) under both searches equal the model's bits -> the AUTO search's stats"""
    want_j, want_d2 = ic.nn_search(queries, targets, max_distance)
    index = dl.NnIndex(ctx, targets, cell_edge=cell_edge)
    try:
        stats = None
        for mode in modes or (dl.NN_AUTO, dl.NN_BRUTE_FORCE):
            j, d2, st = index.query(queries, max_distance, search=mode)
            assert np.array_equal(j, want_j), (mode, np.flatnonzero(j != want_j)[:8])
            assert np.array_equal(bits(d2), bits(want_d2)), (mode, np.flatnonzero(bits(d2) != bits(want_d2))[:8])
            assert st["queries"] == len(want_j)
            assert st["settled_by_grid"] + st["settled_by_brute_force"] + st["non_finite"] == len(want_j)
            if mode == dl.NN_BRUTE_FORCE:
                assert st["settled_by_grid"] == 0
            else:
                stats = st
        return stats
    finally:
        index.close()


def cloud_points(rng, n):
    """A wall, a floor and scattered points: surfaces like a scan's, and empty space between"""
    kind = rng.randint(0, 3, n)
    p = rng.uniform(-20.0, 20.0, (n, 3))
    p[kind == 0, 2] = -1.8 + 0.01 * rng.standard_normal((kind == 0).sum())
    p[kind == 1, 0] = 12.0 + 0.01 * rng.standard_normal((kind == 1).sum())
    return p.astype(np.float32)


@pytest.mark.parametrize("num_targets", [1, 2, 63, 64, 65, 1025, 4097])
def test_search_sizes(dl, ctx, num_targets):
    rng = np.random.RandomState(num_targets)
    targets = cloud_points(rng, num_targets)
    for num_queries in (0, 1, 65, 4097):
        queries = cloud_points(rng, num_queries) + np.float32(0.05)
        check_search(dl, ctx, targets, queries)
        check_search(dl, ctx, targets, queries, max_distance=1.5)


def test_search_every_target_in_one_cell(dl, ctx):
    rng = np.random.RandomState(5)
    targets, queries = cloud_points(rng, 700), cloud_points(rng, 300)
    index = dl.NnIndex(ctx, targets, cell_edge=1e6)
    assert index.memory_stats()["cells"] == 1
    index.close()
    st = check_search(dl, ctx, targets, queries, cell_edge=1e6)
    assert st["settled_by_grid"] == 300  # the shell 0 holds the whole grid
    same = np.tile(np.float32([[1.5, -2.0, 0.25]]), (100, 1))  # a box without extent
    check_search(dl, ctx, same, queries)


def lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_search_lattice_ties(dl, ctx):
    """An integer lattice with one target a cell (edge 1, faces on the integers + 0): queries at the cell centres tie
    eight ways (d2 = 0.75), queries on faces four ways and on edges two ways; the lowest index wins everywhere."""
    targets = lattice(6)
    centres = lattice(5) + np.float32(0.5)
    faces = centres.copy()
    faces[:, 0] -= np.float32(0.5)  # (i, j + 0.5, k + 0.5): on a cell face, four nearest lattice points
    queries = np.concatenate([centres, faces])
    want_j, want_d2 = ic.nn_search(queries, targets)
    assert (want_d2[:len(centres)] == 0.75).all() and (want_d2[len(centres):] == 0.5).all()
    i = np.rint(centres - 0.5).astype(np.int64)
    assert np.array_equal(want_j[:len(centres)], (i[:, 0] * 6 + i[:, 1]) * 6 + i[:, 2])  # the corner with the lowest index
    for edge in (1.0, 0.5, 2.5, 0.0):
        check_search(dl, ctx, targets, queries, cell_edge=edge)
    shuffled = np.random.RandomState(2).permutation(len(targets))  # ties go to the lowest INDEX, wherever the point lies
    check_search(dl, ctx, targets[shuffled], queries, cell_edge=1.0)


def test_search_two_clusters_use_both_paths(dl, ctx):
    """Two clusters 40 m apart and queries between them: the near ones settle in the grid, the far ones -- more than
    DLIOM_NN_MAX_SHELLS cells from any point -- in the brute-force scan."""
    rng = np.random.RandomState(9)
    a = rng.uniform(-1.0, 1.0, (600, 3)).astype(np.float32)
    b = (rng.uniform(-1.0, 1.0, (600, 3)) + [40.0, 0.0, 0.0]).astype(np.float32)
    targets = np.concatenate([a, b])
    x = np.linspace(-1.0, 41.0, 500)
    queries = np.stack([x, rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 500)], axis=1).astype(np.float32)
    st = check_search(dl, ctx, targets, queries, max_distance=30.0, cell_edge=0.5)
    print("two clusters:", st)
    assert st["settled_by_grid"] > 0 and st["settled_by_brute_force"] > 0
    assert st["settled_by_grid"] + st["settled_by_brute_force"] == 500
    st = check_search(dl, ctx, targets, queries, max_distance=0.75, cell_edge=0.5)  # the bound ends every walk
    assert st["settled_by_grid"] == 500


def test_search_distance_bound_is_inclusive(dl, ctx):
    """A query outside the box at exactly max_distance from a lattice point is kept (d2 = 9 <= 3 * 3); one float above
    it is dropped."""
    targets = lattice(4)
    at = np.float32([[6.0, 1.0, 2.0], [1.0, -3.0, 2.0], [2.0, 1.0, 6.0]])  # 3 m beyond the faces x = 3, y = 0, z = 3
    above = at.copy()
    above[0, 0] = np.nextafter(np.float32(6.0), np.float32(7.0))
    above[1, 1] = np.nextafter(np.float32(-3.0), np.float32(-4.0))
    above[2, 2] = np.nextafter(np.float32(6.0), np.float32(7.0))
    want_j, want_d2 = ic.nn_search(np.concatenate([at, above]), targets, 3.0)
    assert (want_d2[:3] == 9.0).all() and (want_j[:3] >= 0).all() and (want_j[3:] == -1).all()
    for edge in (1.0, 0.0, 10.0):
        check_search(dl, ctx, targets, np.concatenate([at, above]), max_distance=3.0, cell_edge=edge)


def test_search_non_finite_points(dl, ctx):
    rng = np.random.RandomState(4)
    targets, queries = cloud_points(rng, 500), cloud_points(rng, 200)
    targets[::7, 0] = np.nan
    targets[3::11, 2] = np.inf
    targets[5::13, 1] = -np.inf
    queries[::5, 1] = np.nan
    queries[1::9, 0] = np.inf
    st = check_search(dl, ctx, targets, queries)
    assert st["non_finite"] == int((~np.isfinite(queries).all(axis=1)).sum())
    index = dl.NnIndex(ctx, targets)
    m = index.memory_stats()
    index.close()
    assert m["points"] == 500 and m["finite_points"] == int(np.isfinite(targets).all(axis=1).sum())
    nothing = np.full((10, 3), np.nan, np.float32)  # no finite target: no neighbour anywhere
    st = check_search(dl, ctx, nothing, queries)


def test_search_points_an_ulp_from_cell_faces(dl, ctx):
    """The stop rule's adversary: with the box's corner at the origin and edge 1 the cell faces are the integers.  Targets
    sit one float below, on and one float above faces, queries likewise: a target just across a face -- or a whole cell
    and an ulp away -- is the nearest for many of them, and the computed d2 rounds below the real distance for some."""
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))  # noqa: E731
    down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    near = [f(v) for v in (1.0, 2.0, 3.0, 4.0) for f in (down, np.float32, up)]
    g = np.array([0.0] + near + [5.0], np.float32)
    targets = np.stack(np.meshgrid(g, g[::2], g[::3], indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.RandomState(8)
    q = rng.choice(g, (3000, 3)).astype(np.float32)
    q[1000:2000] += rng.choice(np.float32([0.5, -0.5, 1.0, -1.0, 0.0]), (1000, 3))  # mid-cell and a cell away, outside too
    q[2000:] = rng.choice(np.concatenate([g, g + np.float32(0.5)]), (1000, 3))
    for edge in (1.0, 0.5, 0.25):
        st = check_search(dl, ctx, targets, q, cell_edge=edge)
    sparse = targets[rng.choice(len(targets), 40, replace=False)]  # few targets: walks of several shells
    for edge in (1.0, 0.5):
        st = check_search(dl, ctx, sparse, q, cell_edge=edge)
        print("sparse", edge, st)


# ---- one iteration ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moved():
    return ic.moved_copy(0.3, 2.0, seed=3)


def options_of(dl, o):
    return dl.icp_options(**{k: o[k] for k in ic.DEFAULTS})


def test_step_equals_model(dl, ctx, moved):
    source, target, _ = moved
    assert (len(source), len(target)) == (877, 1753)
    want = ic.step(source, target)
    index = dl.NnIndex(ctx, target)
    got = dl.Icp(index).step(source)
    index.close()
    assert np.array_equal(got["j"], want["j"]) and np.array_equal(bits(got["d2"]), bits(want["d2"]))
    assert got["n"] == want["n"] == 877
    for name in ("sums", "R", "t"):
        assert np.array_equal(bits(got[name]), bits(want[name])), (name, got[name], want[name])


# ---- alignments ---------------------------------------------------------------------------------------------------------------
def check_align(dl, ctx, source, target, o, guess=None, search=None):
    want = ic.align(source, target, guess, o)
    index = dl.NnIndex(ctx, target)
    try:
        opts = options_of(dl, o)
        if search is not None:
            opts.search = search
        got, aligned = dl.Icp(index, opts).align(source, guess, want_aligned=True)
    finally:
        index.close()
    print("iterations", got["iterations"], "reason", got["reason"], "n", got["correspondences"], "mse", got["mse"], "fitness",
          got["fitness_score"], "read-backs", got["read_backs"], "grid", got["settled_by_grid"], "brute force",
          got["settled_by_brute_force"])
    for name in ("converged", "reason", "iterations", "correspondences", "fitness_count"):
        assert got[name] == want[name], (name, got[name], want[name])
    assert np.array_equal(bits(got["transform"]), bits(want["transform"]))
    for name in ("mse", "fitness_score"):
        assert np.array_equal(bits(np.float64(got[name])), bits(np.float64(want[name]))), (name, got[name], want[name])
    assert same_bits(aligned, want["aligned"])  # the aligned cloud is the model's final p_i
    assert got["read_backs"] == want["iterations"] + 1 + (1 if want["reason"] == ic.NO_CORRESPONDENCES else 0)
    return got, want


@pytest.mark.parametrize("distance", [30.0, 3.0])
def test_align_moved_copy_both_presets(dl, ctx, moved, distance):
    source, target, _ = moved
    got, _ = check_align(dl, ctx, source, target, ic.options(max_correspondence_distance=distance))
    assert got["converged"] == 1 and got["reason"] == dl.ICP_TRANSFORM
    check_align(dl, ctx, source, target, ic.options(max_correspondence_distance=distance), search=dl.NN_BRUTE_FORCE)


@pytest.mark.parametrize("distance", [30.0, 3.0])
def test_align_two_different_scans(dl, ctx, distance):
    target, source = ic.ground_scan(0.30), ic.ground_scan(0.35)
    got, _ = check_align(dl, ctx, source, target, ic.options(max_correspondence_distance=distance))
    assert got["reason"] == dl.ICP_TRANSFORM and 4 <= got["iterations"] <= 6


def test_align_one_iteration_ends_on_iterations(dl, ctx, moved):
    source, target, _ = moved
    got, _ = check_align(dl, ctx, source, target, ic.options(maximum_iterations=1))
    assert (got["converged"], got["reason"], got["iterations"]) == (1, dl.ICP_ITERATIONS, 1)


def test_align_too_few_correspondences(dl, ctx, moved):
    source, target, _ = moved
    got, want = check_align(dl, ctx, source, target, ic.options(max_correspondence_distance=1e-4))
    assert (got["converged"], got["reason"], got["iterations"]) == (0, dl.ICP_NO_CORRESPONDENCES, 0) and got["correspondences"] < 3
    assert np.array_equal(got["transform"], np.eye(4)) and got["mse"] == np.inf and got["fitness_count"] == 877


def test_align_with_a_guess_and_non_finite_points(dl, ctx, moved):
    source, target, motion = moved
    source, target = source.copy(), target.copy()
    source[::50, 1] = np.nan
    target[::40, 0] = np.inf
    guess = ic.pose_matrix(ic.synth.perturb_pose(ic.IDENTITY7, 0.05, 0.5, seed=11))
    got, _ = check_align(dl, ctx, source, target, ic.options(), guess=guess)
    assert got["converged"] == 1 and got["fitness_count"] == int(np.isfinite(source).all(axis=1).sum())


def test_align_twice_gives_the_same_bytes(dl, ctx, moved):
    source, target, _ = moved
    index = dl.NnIndex(ctx, target)
    icp = dl.Icp(index)
    a, pa = icp.align(source, want_aligned=True)
    b, pb = icp.align(source, want_aligned=True)
    index.close()
    other = dl.NnIndex(ctx, target, cell_edge=2.0)  # another grid: the same bytes again
    c, pc = dl.Icp(other).align(source, want_aligned=True)
    other.close()
    for x, px in ((b, pb), (c, pc)):
        assert np.array_equal(bits(x["transform"]), bits(a["transform"])) and same_bits(px, pa)
        for name in ("converged", "reason", "iterations", "correspondences", "fitness_count"):
            assert x[name] == a[name]
        assert bits(np.float64(x["mse"])) == bits(np.float64(a["mse"]))
        assert bits(np.float64(x["fitness_score"])) == bits(np.float64(a["fitness_score"]))


@pytest.mark.parametrize("motion", [(0.3, 2.0), (1.0, 5.0)])
def test_align_recovers_the_motion(dl, ctx, motion):
    """The moved copy returns its motion to within 1e-6 m and 1e-6 in every rotation entry: the project's bound for the
    Ceres pose."""
    source, target, moved_by = ic.moved_copy(motion[0], motion[1], seed=3)
    index = dl.NnIndex(ctx, target)
    got = dl.Icp(index).align(source)
    index.close()
    back = got["transform"] @ moved_by
    print("motion", motion, "iterations", got["iterations"], "|t|", np.linalg.norm(back[:3, 3]), "rotation entries",
          np.abs(back[:3, :3] - np.eye(3)).max())
    assert got["converged"] == 1 and 3 <= got["iterations"] <= 6
    assert np.linalg.norm(back[:3, 3]) <= 1e-6 and np.abs(back[:3, :3] - np.eye(3)).max() <= 1e-6


def test_profiled_alignment_reports_stage_times(dl, ctx, moved):
    source, target, _ = moved
    index = dl.NnIndex(ctx, target)
    plain = dl.Icp(index).align(source)
    assert plain["search_ms"] == plain["reduce_ms"] == plain["transform_ms"] == 0.0
    dl._check(ctx._L.dliom_ctx_set_profiling(ctx.h, 1), "set_profiling")
    try:
        timed = dl.Icp(index).align(source)
    finally:
        dl._check(ctx._L.dliom_ctx_set_profiling(ctx.h, 0), "set_profiling")
        index.close()
    assert timed["search_ms"] > 0 and timed["reduce_ms"] > 0 and timed["transform_ms"] > 0 and timed["solve_ms"] > 0
    assert np.array_equal(bits(timed["transform"]), bits(plain["transform"]))


def test_argument_checks_on_the_device(dl, ctx, moved):
    source, target, _ = moved
    with pytest.raises(dl.DliomError) as e:
        dl.NnIndex(ctx, np.zeros((0, 3), np.float32))  # an empty target is refused
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    index = dl.NnIndex(ctx, target)
    try:
        for bad in (dict(max_correspondence_distance=-1.0), dict(max_correspondence_distance=float("nan")),
                    dict(transformation_epsilon=float("inf")), dict(euclidean_fitness_epsilon=-1e-9), dict(maximum_iterations=-1),
                    dict(min_correspondences=2), dict(search=7)):
            with pytest.raises(dl.DliomError) as e:
                dl.Icp(index, dl.icp_options(**bad)).align(source)
            assert e.value.status == dl.ERR_INVALID_ARGUMENT, bad
        scaled, sheared, nan, mirrored = np.eye(4), np.eye(4), np.eye(4), np.eye(4)
        scaled[:3, :3] *= 1.001
        sheared[0, 1] = 1e-3
        nan[1, 3] = np.nan
        mirrored[2, 2] = -1.0
        for guess in (scaled, sheared, nan, mirrored):
            with pytest.raises(dl.DliomError) as e:
                dl.Icp(index).align(source, guess)
            assert e.value.status == dl.ERR_INVALID_ARGUMENT
        with pytest.raises(dl.DliomError):
            index.query(source, max_distance=-1.0)
    finally:
        index.close()
