"""dliom_nn_index_create_batch on the device: every index against its single-built twin (dliom_nn_index_create) in the
promised memory statistics and in every query's bits, the automatic search against the CPU model
(tests/icp_common.py::nn_search), and the statistics against the Python statement of the schedule
(tests/nn_index_batch_common.py).  Bit equality everywhere: there is no tolerance in this file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_batch_common as bc  # noqa: E402
import icp_common as ic  # noqa: E402
import ndt_batch_common as nbc  # noqa: E402
import nn_index_batch_common as nb  # noqa: E402

pytestmark = pytest.mark.gpu

MEMORY_FIELDS = ("points", "finite_points", "cells", "dims", "cell_edge", "index_bytes")
COUNTERS = ("queries", "non_finite", "settled_by_grid", "settled_by_brute_force")
STAGES = ("box_ms", "sort_ms", "alloc_ms")


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


def answers(dl, index, name):
    """every query set under both search modes -> {(set, mode): (j, d2, counters)}"""
    out = {}
    for which in nb.QUERY_SETS:
        for mode in (dl.NN_AUTO, dl.NN_BRUTE_FORCE):
            j, d2, st = index.query(nb.queries(name, which), search=mode)
            out[(which, mode)] = (j.copy(), d2.copy(), tuple(st[k] for k in COUNTERS))
    return out


@pytest.fixture(scope="module")
def zoo(dl, ctx):
    """name -> dict(cloud, and per edge the single-built twin's memory statistics and answers), built once by
    dliom_nn_index_create; the CPU model's answers under "model" """
    out = {}
    for name in nb.NAMES:
        cloud = dl.PointCloud(ctx, nb.ZOO[name])
        out[name] = dict(cloud=cloud, twins={}, model={w: ic.nn_search(nb.queries(name, w), nb.ZOO[name]) for w in nb.QUERY_SETS})
    yield out
    for name in nb.NAMES:
        out[name]["cloud"].close()


def twin(dl, ctx, zoo, name, edge=0.0, search=0):
    """the single-built index of a zoo cloud, as what a test compares against (made on first use, never changed)"""
    twins = zoo[name]["twins"]
    if (edge, search) not in twins:
        single = dl.NnIndex(ctx, zoo[name]["cloud"], edge, search)
        try:
            twins[(edge, search)] = dict(stats=single.memory_stats(), answers=answers(dl, single, name))
        finally:
            single.close()
    return twins[(edge, search)]


def check_index(dl, ctx, zoo, index, name, edge=0.0, search=0):
    """a batch-built index of the zoo's cloud `name` against its single-built twin, the grid's model and the search's model"""
    want, m = twin(dl, ctx, zoo, name, edge, search), nb.model(name, edge)
    stats = index.memory_stats()
    assert [stats[f] for f in MEMORY_FIELDS] == [want["stats"][f] for f in MEMORY_FIELDS], (name, stats, want["stats"])
    assert (stats["points"], stats["finite_points"], stats["cells"], stats["dims"]) == (m["points"], m["finite_points"], m["cells"], m["dims"])
    assert stats["cell_edge"] == m["cell_edge"] and stats["scratch_bytes"] == 0  # no scratch until the first call
    got = answers(dl, index, name)
    for key, (j, d2, counters) in want["answers"].items():
        assert np.array_equal(got[key][0], j) and bc.same_bits(got[key][1], d2) and got[key][2] == counters, (name, key)
    for which in nb.QUERY_SETS:  # the automatic path against the CPU model (both modes are equal to the twin's, hence to each other's)
        j, d2 = zoo[name]["model"][which]
        key = (which, dl.NN_AUTO if search == 0 else dl.NN_BRUTE_FORCE)
        assert np.array_equal(got[key][0], j) and bc.same_bits(got[key][1], d2), (name, which)
    # a target point finds itself, or the lowest index among its duplicates, at distance 0
    j, d2, _ = got[("self", dl.NN_AUTO)]
    finite = np.isfinite(nb.ZOO[name]).all(axis=1)
    assert (d2[finite] == 0).all() and (j[finite] <= np.flatnonzero(finite)).all() and (j[~finite] == -1).all()
    assert np.array_equal(nb.ZOO[name][j[finite]], nb.ZOO[name][finite])


def check_call(dl, ctx, zoo, names, limits=None, edge=0.0, search=0):
    """one call on the zoo's clouds `names`: every index, the statistics and the context's counters -> the statistics"""
    lim = limits if limits is not None else dl.nn_index_batch_default_limits()
    models = [nb.model(n, edge) for n in names]
    want = nb.expected_stats([m["points"] for m in models], [m["finite_points"] for m in models], [m["cells"] for m in models],
                             lim.max_indices_in_flight, lim.max_points_in_flight, lim.max_cells_in_flight)
    before = (ctx.read_backs(), ctx.synchronizations())
    indices, stats = dl.nn_indices_batch(ctx, [zoo[n]["cloud"] for n in names], edge, search, limits)
    try:
        after = (ctx.read_backs(), ctx.synchronizations())
        print(names, stats)
        assert (after[0] - before[0], after[1] - before[1]) == (want["read_backs"], want["synchronizations"])
        assert {k: stats[k] for k in want} == want
        assert stats["scratch_bytes"] >= 4 * max(m["points"] for m in models) and all(stats[k] == 0.0 for k in STAGES)
        assert len(indices) == len(names)
        for index, name in zip(indices, names):
            check_index(dl, ctx, zoo, index, name, edge, search)
    finally:
        for index in indices:
            index.close()
    return stats


# ---- equality with the single build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 17])
def test_batch_equals_singles_and_model(dl, ctx, zoo, count):
    """17: the whole zoo and three of it again, the equal-box neighbours side by side"""
    stats = check_call(dl, ctx, zoo, nb.first_k(count))
    assert (stats["chunks"], stats["cell_runs"], stats["read_backs"], stats["max_in_flight"]) == (1, 1, 1, count)


@pytest.mark.parametrize("edge", nb.EDGES[1:])
def test_given_cell_edges(dl, ctx, zoo, edge):
    """0.37 m, and 1e-6 m, which every cloud with an extent grows to the cell cap: an index's cells outnumber its points, so the
    scatter's launch is sized by the cells"""
    names = ["n257", "same2", "twin_a", "twin_b", "none", "lattice"]
    stats = check_call(dl, ctx, zoo, names, edge=edge)
    assert stats["chunks"] == 1
    if edge == 1e-6:
        assert stats["cells"] > 4 * (1 << 20) and nb.model("n257", edge)["cells"] > (1 << 20) and nb.model("same2", edge)["cells"] == 1


def test_an_index_that_searches_by_brute_force(dl, ctx, zoo):
    check_call(dl, ctx, zoo, ["n2049", "mixed", "far"], search=dl.NN_BRUTE_FORCE)


# ---- order and repetition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [["n257", "n257"], ["none", "line", "n256"], ["line", "none", "n256"], ["line", "n256", "none"], ["none"],
                                   ["twin_b", "twin_a", "twin_b"]],
                         ids=["twice", "no-finite-first", "no-finite-middle", "no-finite-last", "no-finite-alone", "equal-boxes"])
def test_order_and_repetition(dl, ctx, zoo, names):
    stats = check_call(dl, ctx, zoo, names)
    assert stats["chunks"] == 1 and stats["read_backs"] == 1


FIVE = ["n2049", "none", "far", "lattice", "plane"]


@pytest.mark.parametrize("order", ["identity", "reversed", "random"])
def test_any_order_gives_the_same_indices(dl, ctx, zoo, order):
    names = {"identity": FIVE, "reversed": FIVE[::-1], "random": [FIVE[i] for i in np.random.RandomState(8).permutation(5)]}[order]
    assert sorted(names) == sorted(FIVE) and (order == "identity" or names != FIVE)
    check_call(dl, ctx, zoo, names)


# ---- limits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_indices", [1, 2, 256])
def test_limit_on_indices_in_flight(dl, ctx, zoo, max_indices):
    stats = check_call(dl, ctx, zoo, FIVE, dl.nn_index_batch_default_limits(max_indices_in_flight=max_indices))
    assert stats["chunks"] == stats["read_backs"] == stats["synchronizations"] == {1: 5, 2: 3, 256: 1}[max_indices]


@pytest.mark.parametrize("cut", ["one_point", "one_less_than_two_clouds", "two_clouds", "most"])
def test_limit_on_points_in_flight(dl, ctx, zoo, cut):
    sizes = [len(nb.ZOO[n]) for n in FIVE]
    max_points = {"one_point": 1, "one_less_than_two_clouds": sizes[1] + sizes[2] - 1, "two_clouds": sizes[1] + sizes[2], "most": 1 << 30}[cut]
    stats = check_call(dl, ctx, zoo, FIVE, dl.nn_index_batch_default_limits(max_points_in_flight=max_points))
    # n2049 alone; then none + far only when both fit: the chunk closes in the middle of the list
    assert stats["chunks"] == len(nb.chunks(sizes, 64, max_points)) == {"one_point": 5, "one_less_than_two_clouds": 5, "two_clouds": 4, "most": 1}[cut]


@pytest.mark.parametrize("cut", ["one_cell", "splits", "most"])
def test_limit_on_cells_in_flight(dl, ctx, zoo, cut):
    cells = [nb.model(n)["cells"] for n in FIVE]
    max_cells = {"one_cell": 1, "splits": cells[0] + 1 + cells[1] + 1, "most": 1 << 30}[cut]
    stats = check_call(dl, ctx, zoo, FIVE, dl.nn_index_batch_default_limits(max_cells_in_flight=max_cells))
    runs = nb.cell_runs(cells, max_cells)
    assert stats["chunks"] == stats["read_backs"] == 1  # runs add launches, never read-backs
    assert stats["cell_runs"] == len(runs) and {"one_cell": len(runs) == 5, "splits": 1 < len(runs) < 5 and runs[0] == (0, 2),
                                                "most": len(runs) == 1}[cut]


def test_every_limit_at_its_ends_together(dl, ctx, zoo):
    lim = dl.nn_index_batch_default_limits
    stats = check_call(dl, ctx, zoo, FIVE, lim(max_indices_in_flight=1, max_points_in_flight=1, max_cells_in_flight=1))
    assert (stats["chunks"], stats["cell_runs"]) == (5, 5)
    stats = check_call(dl, ctx, zoo, FIVE, lim(max_indices_in_flight=256, max_points_in_flight=1 << 30, max_cells_in_flight=1 << 30))
    assert (stats["chunks"], stats["cell_runs"]) == (1, 1)
    stats = check_call(dl, ctx, zoo, nb.first_k(17), lim(max_indices_in_flight=2, max_cells_in_flight=600))
    assert stats["chunks"] == 9 and stats["cell_runs"] > 9


# ---- use -----------------------------------------------------------------------------------------------------------------------------
def test_alignments_on_batch_built_indices(dl, ctx):
    """dliom_icp_align, dliom_icp_align_batch and dliom_ndt_align with a fitness index give on a batch-built index the bytes they
    give on a single-built one"""
    scene = nbc.scene_points()
    rng = np.random.RandomState(9)
    moved = (scene[rng.permutation(len(scene))[:2049]] + np.float32([0.1, -0.05, 0.02])).astype(np.float32)
    other = (scene + np.float32([0.5, 0.0, 0.0])).astype(np.float32)
    o = dl.icp_options(maximum_iterations=6)
    no = dl.ndt_options(maximum_iterations=4)
    single = dl.NnIndex(ctx, scene)
    target = dl.NdtTarget(ctx, scene, no)
    built, _ = dl.nn_indices_batch(ctx, [other, scene, other])
    try:
        want = dl.Icp(single, o).align(moved, None, want_aligned=True)
        got = dl.Icp(built[1], o).align(moved, None, want_aligned=True)
        assert bc.same_result(got[0], want[0]) == [] and bc.same_bits(got[1], want[1]) and want[0]["iterations"] >= 1
        pairs = lambda index: [(index, moved, None), (index, moved[:700], nbc.MOVED_GUESS)]  # noqa: E731
        want_batch, _ = dl.icp_align_batch(ctx, pairs(single), o)
        got_batch, _ = dl.icp_align_batch(ctx, pairs(built[1]), o)
        for a, b in zip(got_batch, want_batch):
            assert bc.same_result(a, b) == []
        want_ndt = dl.Ndt(target, no, single).align(moved, want_aligned=True)
        got_ndt = dl.Ndt(target, no, built[1]).align(moved, want_aligned=True)
        assert nbc.same_result(got_ndt[0], want_ndt[0]) == [] and bc.same_bits(got_ndt[1], want_ndt[1])
        assert want_ndt[0]["fitness_count"] > 1000
    finally:
        for t in built + [single, target]:
            t.close()


# ---- lifetime and work space -------------------------------------------------------------------------------------------------------
def test_indices_are_destroyed_on_their_own_and_outlive_their_clouds(dl, ctx, zoo):
    names = ["n2049", "far", "lattice", "twin_a"]
    clouds = [dl.PointCloud(ctx, nb.ZOO[n]) for n in names]
    indices, _ = dl.nn_indices_batch(ctx, clouds)
    for c in clouds:
        c.close()
    indices[2].close()
    indices[0].close()
    check_index(dl, ctx, zoo, indices[3], "twin_a")
    check_index(dl, ctx, zoo, indices[1], "far")
    indices[3].close()
    stats = indices[1].memory_stats()
    assert stats["scratch_bytes"] > 0  # its queries' scratch, its own
    indices[1].close()
    indices[1].close()  # closing twice is harmless, as for a single-built index


def test_two_calls_in_a_row_and_arrays_as_clouds(dl, ctx, zoo):
    """A smaller call after a larger one on the same work space, then from numpy arrays, one of them named twice"""
    big = check_call(dl, ctx, zoo, ["n2049", "far", "plane"], edge=1e-6)
    small = check_call(dl, ctx, zoo, ["n255", "p1"])
    assert small["scratch_bytes"] < big["scratch_bytes"]
    a = nb.ZOO["n256"]
    indices, stats = dl.nn_indices_batch(ctx, [a, nb.ZOO["mixed"], a])
    try:
        assert stats["indices"] == 3 and indices[0].h.value != indices[2].h.value  # each mention an index of its own
        for index, name in zip(indices, ["n256", "mixed", "n256"]):
            check_index(dl, ctx, zoo, index, name)
    finally:
        for index in indices:
            index.close()


# ---- refusals and profiling ----------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(dl, ctx, zoo):
    L = ctx._L
    o, lim = dl.NnIndexOptions(0.0, dl.NN_AUTO, 0), dl.nn_index_batch_default_limits()
    other_ctx = dl.Context(0)
    foreign = dl.PointCloud(other_ctx, nb.ZOO["p1"])
    empty = dl.PointCloud(ctx, np.zeros((0, 3), np.float32))
    good = [zoo["p1"]["cloud"].h, zoo["n257"]["cloud"].h, zoo["none"]["cloud"].h]
    sentinel = 0x5a5a
    try:
        def call(handles, count=None, options=o, limits=lim, ctx_h=ctx.h, clouds="own", with_out=True):
            table = (C.c_void_p * max(len(handles), 1))(*[h if h is None else C.c_void_p(h.value if hasattr(h, "value") else h) for h in handles])
            out = (C.c_void_p * 4)(*[sentinel] * 4)
            before = (ctx.read_backs(), ctx.synchronizations())
            status = L.dliom_nn_index_create_batch(ctx_h, table if clouds == "own" else None, len(handles) if count is None else count,
                                                   None if options is None else C.byref(options),
                                                   None if limits is None else C.byref(limits), out if with_out else None, None)
            ran = (ctx.read_backs(), ctx.synchronizations()) != before
            got = [out[k] for k in range(4)]
            if status == dl.OK:
                for k in range(len(handles) if count is None else count):
                    L.dliom_nn_index_destroy(C.c_void_p(got[k]))
            return status, ran, got

        bad = dl.ERR_INVALID_ARGUMENT
        null3 = [None, None, None, sentinel]  # every out[i] of the call is NULL; what lies behind is not touched
        status, ran, got = call(good)
        assert status == dl.OK and ran and all(got[:3]) and got[3] == sentinel
        assert call(good, ctx_h=None) == (bad, False, null3)
        assert call(good, clouds=None) == (bad, False, null3)
        assert call(good, with_out=False)[:2] == (bad, False)
        assert call(good, count=-1) == (bad, False, [sentinel] * 4)
        for wrong in ((-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), (0.0, 2, 0), (0.0, -1, 0), (0.0, 0, 1)):
            assert call(good, options=dl.NnIndexOptions(*wrong)) == (bad, False, null3), wrong
        for wrong in (dict(max_indices_in_flight=0), dict(max_indices_in_flight=257), dict(reserved=1), dict(max_points_in_flight=0),
                      dict(max_points_in_flight=-5), dict(max_points_in_flight=(1 << 30) + 1), dict(max_cells_in_flight=0),
                      dict(max_cells_in_flight=(1 << 30) + 1)):
            assert call(good, limits=dl.nn_index_batch_default_limits(**wrong)) == (bad, False, null3), wrong
        # a bad cloud in the LAST place fails the call before the first cloud runs
        assert call(good[:2] + [None]) == (bad, False, null3)
        assert call(good[:2] + [foreign.h]) == (bad, False, null3)
        assert call(good[:2] + [empty.h]) == (bad, False, null3)
        # count == 0 succeeds and launches nothing; options and limits NULL are the defaults; the ranges' ends are inside
        assert call(good, count=0) == (dl.OK, False, [sentinel] * 4)
        assert call(good, limits=None)[0] == dl.OK and call(good, options=None)[0] == dl.OK
        assert call(good, limits=dl.nn_index_batch_default_limits(max_indices_in_flight=256, max_points_in_flight=1 << 30,
                                                                  max_cells_in_flight=1 << 30))[0] == dl.OK
        indices, stats = dl.nn_indices_batch(ctx, [])
        assert indices == [] and stats == dict(indices=0, chunks=0, cell_runs=0, points=0, finite_points=0, cells=0, read_backs=0,
                                               synchronizations=0, max_in_flight=0, scratch_bytes=0, box_ms=0.0, sort_ms=0.0, alloc_ms=0.0)
    finally:
        empty.close()
        foreign.close()
        other_ctx.close()


def test_profiled_build_reports_stage_times(dl, ctx, zoo):
    names = ["n2049", "far", "twin_a"]
    ctx.set_profiling(1)
    try:
        indices, stats = dl.nn_indices_batch(ctx, [zoo[n]["cloud"] for n in names])
    finally:
        ctx.set_profiling(0)
    try:
        assert all(stats[k] > 0 for k in STAGES) and (stats["read_backs"], stats["synchronizations"], stats["cell_runs"]) == (1, 1, 1)
        for index, n in zip(indices, names):
            check_index(dl, ctx, zoo, index, n)
    finally:
        for index in indices:
            index.close()


# ---- the C++ adapters ------------------------------------------------------------------------------------------------------------------
def test_adapter_program(dl, tmp_path):
    """tests/cpp/nn_index_batch_adapter.cc builds with g++ -Wall -Werror and holds: BuildNnIndices gives, cloud by cloud, an index
    that answers as dliom_nn_index_create's does, in one chunk with one read-back; AlignPairs and AlignPairsNdt give under
    kBatched the results and clouds they give under kOneByOne, with one build read-back a chunk in place of one a target; the
    two generators' text is byte-equal under both."""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path / "nn_index_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "nn_index_batch_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
