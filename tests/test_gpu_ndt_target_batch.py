"""dliom_ndt_target_create_batch on the device: every target against its single-built twin (dliom_ndt_target_create) and
against the CPU model's cells (tests/ndt_common.py::build_cells), bits; the statistics against the Python statement of the
schedule (tests/ndt_target_batch_common.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_common as ic  # noqa: E402
import ndt_batch_common as bc  # noqa: E402
import ndt_common as nd  # noqa: E402
import ndt_target_batch_common as tb  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC_P = [0.4, -0.3, 0.2, 0.05, -0.08, 0.11]
KINDS = (nd.EVAL_GRADIENT, nd.EVAL_ALL, nd.EVAL_HESSIAN)
COUNT_FIELDS = ("points", "kept_points", "cells", "valid_cells", "target_bytes")


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
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN standing for any other (tests/test_gpu_ndt.py)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def evaluations(dl, target, source):
    """the valid cells as the device holds them: dliom_ndt_evaluate at a generic p under the three kinds"""
    return [dl.Ndt(target).evaluate(source, GENERIC_P, what) for what in KINDS]


@pytest.fixture(scope="module")
def zoo(dl, ctx):
    """name -> dict(cloud, single target's cells, counts and evaluations), built once by dliom_ndt_target_create; and the
    evaluations' source, 2049 points over the zoo's cells"""
    rng = np.random.RandomState(21)
    source = dl.PointCloud(ctx, rng.uniform([-4.0, -3.0, -2.0], [18.0, 5.0, 2.5], (2049, 3)).astype(np.float32))
    out = {"source": source}
    for name in tb.NAMES:
        cloud = dl.PointCloud(ctx, tb.ZOO[name])
        single = dl.NdtTarget(ctx, cloud)
        try:
            out[name] = dict(cloud=cloud, cells=single.cells(), stats=single.memory_stats(), evaluations=evaluations(dl, single, source))
        finally:
            single.close()
    assert sum(e["pairs"] for name in tb.NAMES for e in out[name]["evaluations"]) > 1000  # the source does meet the cells
    yield out
    for name in tb.NAMES:
        out[name]["cloud"].close()
    source.close()


def check_cells(got, want):
    """tests/test_gpu_ndt.py::check_cells' comparison"""
    assert np.array_equal(got["index"], want["index"])
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["valid"], want["valid"])
    assert same_bits(got["mean"], want["mean"]), np.flatnonzero((bits(got["mean"]) != bits(want["mean"])).any(axis=1))[:8]
    assert same_bits(got["icov"], want["icov"]), np.flatnonzero((bits(got["icov"]) != bits(want["icov"])).any(axis=1))[:8]


def check_target(dl, zoo, target, name, read_backs, evaluate=True):
    """a batch-built target of the zoo's cloud `name` against its single-built twin and the model, in every promised field"""
    twin, model = zoo[name], tb.model(name)
    got, stats = target.cells(), target.memory_stats()
    check_cells(got, twin["cells"])
    check_cells(got, model)
    assert [stats[f] for f in COUNT_FIELDS] == [twin["stats"][f] for f in COUNT_FIELDS]
    assert (stats["points"], stats["kept_points"], stats["cells"], stats["valid_cells"]) == \
        (len(tb.ZOO[name]), model["kept_points"], len(model["n"]), int(model["valid"].sum()))
    assert stats["read_backs"] == read_backs and stats["build_ms"] == 0.0
    if evaluate:
        for a, b in zip(evaluations(dl, target, zoo["source"]), twin["evaluations"]):
            assert a["pairs"] == b["pairs"] and same_bits([a["score"]], [b["score"]])
            assert same_bits(a["gradient"], b["gradient"]) and same_bits(a["hessian"], b["hessian"])


def check_call(dl, ctx, zoo, names, limits=None, evaluate=True):
    """one call on the zoo's clouds `names`: every target, the statistics and the context's counters -> the statistics"""
    lim = limits if limits is not None else dl.ndt_target_batch_default_limits()
    sizes = [len(tb.ZOO[n]) for n in names]
    models = [tb.model(n) for n in names]
    cells = [len(m["n"]) for m in models]
    want = tb.expected_stats(sizes, [m["kept_points"] for m in models], cells, [int(m["valid"].sum()) for m in models],
                             lim.max_targets_in_flight, lim.max_points_in_flight)
    before = (ctx.read_backs(), ctx.synchronizations())
    targets, stats = dl.ndt_targets_batch(ctx, [zoo[n]["cloud"] for n in names], limits=limits)
    try:
        assert (ctx.read_backs() - before[0], ctx.synchronizations() - before[1]) == (want["read_backs"], want["synchronizations"])
        print(names, stats)
        assert {k: stats[k] for k in want} == want
        assert stats["scratch_bytes"] >= 56 * max(sizes) and stats["sort_ms"] == stats["sums_ms"] == stats["host_ms"] == stats["upload_ms"] == 0.0
        assert len(targets) == len(names)
        per_target = tb.target_read_backs(sizes, cells, lim.max_targets_in_flight, lim.max_points_in_flight)
        for target, name, rb in zip(targets, names, per_target):
            check_target(dl, zoo, target, name, rb, evaluate)
    finally:
        for t in targets:
            t.close()
    return stats


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 17])
def test_batch_equals_singles_and_model(dl, ctx, zoo, count):
    """1 (the chain without the second sort), 2 and 3 (one and two slot bits), 17 (five bits; the zoo and six of it again)"""
    stats = check_call(dl, ctx, zoo, tb.first_k(count))
    assert (stats["chunks"], stats["read_backs"], stats["max_in_flight"]) == (1, 2, count)


# ---- boundaries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [["one", "one"], ["lengths", "lengths"], ["degenerate", "none", "degenerate", "none", "degenerate"],
                                   ["none", "faces", "n257"], ["faces", "none", "n257"], ["faces", "n257", "none"]],
                         ids=["one-cell-twice", "lengths-twice", "thrice-around-no-cell", "no-cell-first", "no-cell-middle", "no-cell-last"])
def test_target_boundaries(dl, ctx, zoo, names):
    """Neighbouring targets that end and start on equal keys (the one cell's, or the skip key): no cell is merged or lost
    and the kept counts are each target's own"""
    stats = check_call(dl, ctx, zoo, names)
    assert stats["chunks"] == 1 and stats["read_backs"] == 2


def test_a_chunk_without_any_cell_costs_one_read_back(dl, ctx, zoo):
    stats = check_call(dl, ctx, zoo, ["none"])
    assert (stats["read_backs"], stats["cells"], stats["kept_points"], stats["points"]) == (1, 0, 0, 5)
    stats = check_call(dl, ctx, zoo, ["none", "none", "n1"], dl.ndt_target_batch_default_limits(max_targets_in_flight=2))
    assert (stats["chunks"], stats["read_backs"]) == (2, 1 + 2)


# ---- independence ----------------------------------------------------------------------------------------------------------------------
FIVE = ["lengths", "none", "n257", "degenerate", "one"]


@pytest.mark.parametrize("order", ["identity", "reversed", "random"])
def test_any_order_gives_the_same_targets(dl, ctx, zoo, order):
    names = {"identity": FIVE, "reversed": FIVE[::-1], "random": [FIVE[i] for i in np.random.RandomState(8).permutation(5)]}[order]
    assert sorted(names) == sorted(FIVE) and (order == "identity" or names != FIVE)
    check_call(dl, ctx, zoo, names)


@pytest.mark.parametrize("max_targets", [1, 2, 256])
def test_limit_on_targets_in_flight(dl, ctx, zoo, max_targets):
    stats = check_call(dl, ctx, zoo, FIVE, dl.ndt_target_batch_default_limits(max_targets_in_flight=max_targets), evaluate=False)
    assert stats["chunks"] == {1: 5, 2: 3, 256: 1}[max_targets]
    assert stats["read_backs"] == {1: 2 + 1 + 2 + 2 + 2, 2: 6, 256: 2}[max_targets]


@pytest.mark.parametrize("cut", ["one_point", "smallest_cloud", "one_less_than_two_clouds", "default"])
def test_limit_on_points_in_flight(dl, ctx, zoo, cut):
    sizes = [len(tb.ZOO[n]) for n in FIVE]
    max_points = {"one_point": 1, "smallest_cloud": min(sizes), "one_less_than_two_clouds": sizes[2] + sizes[3] - 1,
                  "default": tb.DEFAULT_MAX_POINTS}[cut]
    stats = check_call(dl, ctx, zoo, FIVE, dl.ndt_target_batch_default_limits(max_points_in_flight=max_points), evaluate=False)
    # one less than n257 + degenerate: none and n257 still share a chunk, degenerate opens the next one
    assert stats["chunks"] == len(tb.chunks(sizes, 64, max_points)) == {"one_point": 5, "smallest_cloud": 5,
                                                                        "one_less_than_two_clouds": 3, "default": 1}[cut]


def test_limit_on_points_in_flight_that_pairs_small_clouds(dl, ctx, zoo):
    names = ["n255", "n256", "n257", "none", "one", "n1"]
    stats = check_call(dl, ctx, zoo, names, dl.ndt_target_batch_default_limits(max_points_in_flight=255 + 256), evaluate=False)
    assert stats["chunks"] == 2 and stats["max_in_flight"] == 4  # 255 + 256 fits exactly; then 257 + 5 + 16 + 1


# ---- use -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [nd.STEP_CLAMPED, nd.STEP_MORE_THUENTE], ids=["clamped", "more-thuente"])
def test_alignments_on_batch_built_targets(dl, ctx, mode):
    """dliom_ndt_align and dliom_ndt_align_batch give on a batch-built target the bits they give on a single-built one"""
    scene = bc.scene_points()
    rng = np.random.RandomState(9)
    moved = (scene[rng.permutation(len(scene))[:2049]] + np.float32([0.1, -0.05, 0.02])).astype(np.float32)
    o = dl.ndt_options(step_mode=mode, maximum_iterations=4)
    other = (scene + np.float32([0.5, 0.0, 0.0])).astype(np.float32)
    single = dl.NdtTarget(ctx, scene, o)
    index = dl.NnIndex(ctx, scene)
    built, _ = dl.ndt_targets_batch(ctx, [other, scene, other], o)
    try:
        want = dl.Ndt(single, o, index).align(moved, want_aligned=True)
        got = dl.Ndt(built[1], o, index).align(moved, want_aligned=True)
        assert bc.same_result(got[0], want[0]) == [] and same_bits(got[1], want[1])
        assert want[0]["iterations"] >= 1 and want[0]["pairs"] > 1000
        pairs = lambda t: [(t, moved, None, index), (t, moved, bc.MOVED_GUESS, None)]  # noqa: E731
        want_batch, _ = dl.ndt_align_batch(ctx, pairs(single), o)
        got_batch, _ = dl.ndt_align_batch(ctx, pairs(built[1]), o)
        for a, b in zip(got_batch, want_batch):
            assert bc.same_result(a, b) == []
    finally:
        for t in built + [single, index]:
            t.close()


def test_targets_are_destroyed_on_their_own_and_outlive_their_clouds(dl, ctx, zoo):
    names = ["lengths", "faces", "sparse", "n2049"]
    clouds = [dl.PointCloud(ctx, tb.ZOO[n]) for n in names]
    targets, _ = dl.ndt_targets_batch(ctx, clouds)
    for c in clouds:
        c.close()
    targets[2].close()
    targets[0].close()
    check_target(dl, zoo, targets[3], "n2049", 2)
    check_target(dl, zoo, targets[1], "faces", 2)
    targets[3].close()
    check_target(dl, zoo, targets[1], "faces", 2)
    targets[1].close()
    targets[1].close()  # closing twice is harmless, as for a single-built target


def test_two_calls_in_a_row_and_arrays_as_clouds(dl, ctx, zoo):
    """A smaller call after a larger one on the same work space, from numpy arrays, one of them named twice"""
    check_call(dl, ctx, zoo, ["lengths", "n2049", "faces"], evaluate=False)
    check_call(dl, ctx, zoo, ["n257", "one"], evaluate=False)
    a = tb.ZOO["n256"]
    targets, stats = dl.ndt_targets_batch(ctx, [a, tb.ZOO["sparse"], a])
    try:
        assert stats["targets"] == 3 and targets[0].h.value != targets[2].h.value  # each mention a target of its own
        for t, name in zip(targets, ["n256", "sparse", "n256"]):
            check_target(dl, zoo, t, name, 2, evaluate=False)
    finally:
        for t in targets:
            t.close()
    coarse, _ = dl.ndt_targets_batch(ctx, [tb.ZOO["faces"], tb.ZOO["lengths"]], dl.ndt_options(resolution=0.3, min_points_per_voxel=3))
    try:
        for t, name in zip(coarse, ["faces", "lengths"]):
            check_cells(t.cells(), tb.model(name, resolution=0.3, min_points_per_voxel=3))
    finally:
        for t in coarse:
            t.close()


# ---- refusals and profiling ------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(dl, ctx, zoo):
    L = ctx._L
    o, lim = dl.ndt_options(), dl.ndt_target_batch_default_limits()
    other_ctx = dl.Context(0)
    foreign = dl.PointCloud(other_ctx, tb.ZOO["one"])
    empty = dl.PointCloud(ctx, np.zeros((0, 3), np.float32))
    good = [zoo["one"]["cloud"].h, zoo["faces"]["cloud"].h, zoo["none"]["cloud"].h]
    sentinel = 0x5a5a
    try:
        def call(handles, count=None, options=o, limits=lim, ctx_h=ctx.h, clouds="own", with_out=True):
            table = (C.c_void_p * max(len(handles), 1))(*[h if h is None else C.c_void_p(h.value if hasattr(h, "value") else h) for h in handles])
            out = (C.c_void_p * 4)(*[sentinel] * 4)
            before = (ctx.read_backs(), ctx.synchronizations())
            status = L.dliom_ndt_target_create_batch(ctx_h, table if clouds == "own" else None, len(handles) if count is None else count,
                                                     None if options is None else C.byref(options),
                                                     None if limits is None else C.byref(limits), out if with_out else None, None)
            ran = (ctx.read_backs(), ctx.synchronizations()) != before
            got = [out[k] for k in range(4)]
            if status == dl.OK:
                for k in range(len(handles) if count is None else count):
                    L.dliom_ndt_target_destroy(C.c_void_p(got[k]))
            return status, ran, got

        bad = dl.ERR_INVALID_ARGUMENT
        null3 = [None, None, None, sentinel]  # every out[i] of the call is NULL; what lies behind is not touched
        status, ran, got = call(good)
        assert status == dl.OK and ran and all(got[:3]) and got[3] == sentinel
        assert call(good, ctx_h=None) == (bad, False, null3)
        assert call(good, clouds=None) == (bad, False, null3)
        assert call(good, with_out=False)[:2] == (bad, False)
        assert call(good, options=None) == (bad, False, null3)
        assert call(good, count=-1) == (bad, False, [sentinel] * 4)
        for wrong in (dict(resolution=0.0), dict(step_size=float("inf")), dict(outlier_ratio=1.0), dict(transformation_epsilon=-1e-9),
                      dict(maximum_iterations=-1), dict(min_points_per_voxel=2), dict(step_mode=2), dict(reserved=1)):
            assert call(good, options=dl.ndt_options(**wrong)) == (bad, False, null3), wrong
        for wrong in (dict(max_targets_in_flight=0), dict(max_targets_in_flight=257), dict(reserved=1), dict(max_points_in_flight=0),
                      dict(max_points_in_flight=-5), dict(max_points_in_flight=(1 << 30) + 1)):
            assert call(good, limits=dl.ndt_target_batch_default_limits(**wrong)) == (bad, False, null3), wrong
        # a bad cloud in the LAST place fails the call before the first cloud runs
        assert call(good[:2] + [None]) == (bad, False, null3)
        assert call(good[:2] + [foreign.h]) == (bad, False, null3)
        assert call(good[:2] + [empty.h]) == (bad, False, null3)
        # count == 0 succeeds and launches nothing; limits NULL are the defaults; the ranges' ends are inside
        assert call(good, count=0) == (dl.OK, False, [sentinel] * 4)
        assert call(good, limits=None)[0] == dl.OK
        assert call(good, limits=dl.ndt_target_batch_default_limits(max_targets_in_flight=256, max_points_in_flight=1 << 30))[0] == dl.OK
        targets, stats = dl.ndt_targets_batch(ctx, [])
        assert targets == [] and stats == dict(targets=0, chunks=0, points=0, kept_points=0, cells=0, valid_cells=0, read_backs=0,
                                               synchronizations=0, max_in_flight=0, scratch_bytes=0, sort_ms=0.0, sums_ms=0.0,
                                               host_ms=0.0, upload_ms=0.0)
    finally:
        empty.close()
        foreign.close()
        other_ctx.close()


def test_profiled_build_reports_stage_times(dl, ctx, zoo):
    names = ["lengths", "faces", "n2049"]
    clouds = [zoo[n]["cloud"] for n in names]
    ctx.set_profiling(1)
    try:
        targets, stats = dl.ndt_targets_batch(ctx, clouds)
    finally:
        ctx.set_profiling(0)
    try:
        assert stats["sort_ms"] > 0 and stats["sums_ms"] > 0 and stats["host_ms"] > 0 and stats["upload_ms"] > 0
        assert (stats["read_backs"], stats["synchronizations"]) == (2, 1)
        for t, n in zip(targets, names):
            check_target(dl, zoo, t, n, 2, evaluate=False)  # build_ms stays 0: the times are the call's
    finally:
        for t in targets:
            t.close()


# ---- the C++ adapter -------------------------------------------------------------------------------------------------------------------
def test_adapter_program(dl, tmp_path):
    """tests/cpp/ndt_target_batch_adapter.cc builds with g++ -Wall -Werror and holds: BuildNdtTargets gives, cloud by cloud,
    what NormalDistributionsTransform::setInputTarget builds (cells, counts, and the alignment on them), in one chunk with two
    read-backs; GenerateGroundTruthNdt's text on the 12-node trajectory is byte-equal to the pair-at-a-time loop for batch
    sizes 1, 3 and 100."""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path / "ndt_target_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "ndt_target_batch_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
