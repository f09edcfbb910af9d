"""dliom_ndt_align_batch on the device: every pair's result and aligned cloud equal dliom_ndt_align's bits, whatever the
chunking, the order and the company of a pair, and the call's statistics are those of the fixed schedule (dliom.h)."""
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

pytestmark = pytest.mark.gpu
MODES = [nd.STEP_CLAMPED, nd.STEP_MORE_THUENTE]
MODE_IDS = ["clamped", "more-thuente"]


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


def options_of(dl, mode, **overrides):
    return dl.ndt_options(**nd.options(step_mode=mode, **overrides))


def singles(dl, pairs, options):
    """dliom_ndt_align pair by pair -> [(result, aligned points)]"""
    return [dl.Ndt(target, options, fitness_index=index).align(source, guess, want_aligned=True)
            for target, source, guess, index in pairs]


def single_read_backs(result, n, index, wanted):
    """What dliom_ndt_align counts: the evaluations, the fitness score's, the norm bound's"""
    evaluations = result["evaluations_with_hessian"] + result["evaluations_without_hessian"]
    return evaluations + (1 if index is not None else 0) + (1 if wanted and n > 0 else 0)


def check_batch(dl, ctx, pairs, options, want, limits=None):
    """One batched call with the clouds and one without, whose results and clouds equal `want` (singles' output) -> the
    statistics of both"""
    before = ctx.read_backs()
    results, stats, clouds = dl.ndt_align_batch(ctx, pairs, options, limits, want_aligned=True)
    assert ctx.read_backs() - before == stats["read_backs"] == stats["steps"]
    assert len(results) == len(clouds) == len(want) == stats["pairs"]
    for i, ((single, points), got, cloud, pair) in enumerate(zip(want, results, clouds, pairs)):
        assert bc.same_result(got, single, read_backs=False) == [], (i, bc.same_result(got, single, False), got, single)
        assert bc.same_bits(cloud, points), i
        evaluations = got["evaluations_with_hessian"] + got["evaluations_without_hessian"]
        assert got["read_backs"] == evaluations + 1
        n = len(points)
        assert single["read_backs"] == single_read_backs(single, n, pair[3], True)
        assert single["read_backs"] - got["read_backs"] == (1 if pair[3] is not None and n > 0 else (-1 if pair[3] is None and n == 0 else 0))
        assert got["evaluate_ms"] == got["reduce_ms"] == got["host_ms"] == 0.0
    assert stats["pair_evaluations"] == sum(r["evaluations_with_hessian"] + r["evaluations_without_hessian"] for r, _ in want)
    assert stats["pair_searches"] == len(pairs) and stats["synchronizations"] == stats["chunks"]
    plain, plain_stats = dl.ndt_align_batch(ctx, pairs, options, limits)  # without the clouds: the same results
    for got, (single, _), pair in zip(plain, want, pairs):
        assert bc.same_result(got, single, read_backs=False) == []
        evaluations = got["evaluations_with_hessian"] + got["evaluations_without_hessian"]
        assert got["read_backs"] == evaluations + (1 if pair[3] is not None else 0)  # no final round without an index
    assert plain_stats["synchronizations"] == 0 and plain_stats["pair_searches"] == sum(1 for p in pairs if p[3] is not None)
    return stats, plain_stats


def expected(model, pairs, sizes, finals, max_pairs, budget):
    return bc.expected_stats([k for _, k in model], finals, [len(p[1]) for p in pairs], sizes, max_pairs, budget)


def stats_equal(got, want):
    assert {k: got[k] for k in want} == want, ({k: got[k] for k in want}, want)


# ---- the zoo ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo(dl, ctx):
    points, pairs = bc.zoo_pairs()
    o = {mode: options_of(dl, mode, **bc.ZOO_OPTIONS) for mode in MODES}
    targets = {name: dl.NdtTarget(ctx, p, o[nd.STEP_CLAMPED]) for name, p in points.items()}
    indices = {name: dl.NnIndex(ctx, p) for name, p in points.items()}
    device = [(targets[name], source, guess, indices[name] if fitness else None) for name, source, guess, fitness in pairs]
    want = {mode: singles(dl, device, o[mode]) for mode in MODES}
    sizes = [dl.ndt_batch_scratch_bytes(len(p[1])) for p in device]
    yield dict(pairs=device, options=o, want=want, sizes=sizes, model={mode: bc.zoo_model(mode) for mode in MODES})
    for t in list(targets.values()) + list(indices.values()):
        t.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("count", [1, 2, 3, 17])
def test_batch_equals_singles(dl, ctx, zoo, count, mode):
    first = {1: 4, 2: 3, 3: 0, 17: 0}[count]  # K = 1 and 2 start at pairs with points; 3 and 17 begin with the empty source
    sl = slice(first, first + count)
    pairs, want, model = zoo["pairs"][sl], zoo["want"][mode][sl], zoo["model"][mode][sl]
    limits = dl.ndt_batch_default_limits(max_pairs_in_flight=256)
    stats, plain = check_batch(dl, ctx, pairs, zoo["options"][mode], want, limits)
    print("K", count, "mode", mode, "stats", stats)
    assert stats["chunks"] == 1 and stats["max_in_flight"] == count
    rounds = [bc.rounds_of(k, True) for _, k in model]
    assert stats["steps"] == max(rounds)  # not their sum: what the call exists for
    stats_equal(stats, expected(model, pairs, zoo["sizes"][sl], [True] * count, 256, limits.max_scratch_bytes))
    stats_equal(plain, expected(model, pairs, zoo["sizes"][sl], [p[3] is not None for p in pairs], 256, limits.max_scratch_bytes))
    if mode == nd.STEP_CLAMPED:
        assert stats["evaluation_launches"][nd.EVAL_GRADIENT] == stats["evaluation_launches"][nd.EVAL_HESSIAN] == 0
    elif count in (2, 17):  # (the first three pairs are short: they evaluate everything every time)
        assert stats["mixed_steps"] > 0 and all(v > 0 for v in stats["evaluation_launches"])
    if count == 17:
        assert len(set(rounds)) > 2 and stats["steps"] < sum(rounds)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_pairs_equal_the_cpu_model(dl, ctx, zoo, mode):
    """Every zoo pair against tests/ndt_common.py (among them pairs 2, 3, 5 and 8: 65, 2047, 2049 and 1 points)"""
    results, _, clouds = dl.ndt_align_batch(ctx, zoo["pairs"], zoo["options"][mode], want_aligned=True)
    for i, (got, cloud, (want, _)) in enumerate(zip(results, clouds, zoo["model"][mode])):
        assert bc.same_result(got, want, read_backs=False) == [], (i, bc.same_result(got, want, False), got, want)
        assert bc.same_bits(cloud, want["aligned"].astype(np.float32).reshape(-1, 3)), i


# ---- pairs that end at different rounds -------------------------------------------------------------------------------------------------
def test_pairs_that_end_at_different_rounds(dl, ctx):
    points = bc.zoo_targets()
    scene = points["scene"]
    moved = (scene[::2] + np.float32([0.12, -0.07, 0.03])).astype(np.float32)
    holes = moved.copy()
    holes[::9, 0] = np.nan
    holes[4::13, 2] = -np.inf
    empty = np.zeros((0, 3), np.float32)
    o = options_of(dl, nd.STEP_MORE_THUENTE, maximum_iterations=1)
    target, nothing, index = dl.NdtTarget(ctx, scene, o), dl.NdtTarget(ctx, points["none"], o), dl.NnIndex(ctx, scene)
    try:
        pairs = [(nothing, moved, None, index), (target, moved, None, index), (target, scene[::3].copy(), None, None),
                 (target, holes, None, index), (target, empty, None, index), (target, moved, bc.MOVED_GUESS, None),
                 (target, moved, None, index)]
        want = singles(dl, pairs, o)
        reasons = [(r["reason"], r["iterations"]) for r, _ in want]
        print("reasons", reasons, "evaluations", [r["evaluations_with_hessian"] + r["evaluations_without_hessian"] for r, _ in want])
        assert reasons[0] == (dl.NDT_ZERO_STEP, 0) and want[0][0]["evaluations_with_hessian"] == 1  # at once
        assert reasons[1] == (dl.NDT_ITERATIONS, 3)  # by the count
        assert reasons[2][0] == dl.NDT_EPSILON  # a copy of target points: by epsilon
        assert want[3][0]["fitness_count"] == int(np.isfinite(holes).all(axis=1).sum())
        assert reasons[4] == (dl.NDT_ZERO_STEP, 0) and want[4][0]["fitness_count"] == 0 and np.isnan(want[4][0]["fitness_score"])
        stats, _ = check_batch(dl, ctx, pairs, o, want)
        evaluations = [r["evaluations_with_hessian"] + r["evaluations_without_hessian"] for r, _ in want]
        assert len(set(evaluations)) >= 3 and stats["chunks"] == 1 and stats["steps"] == max(evaluations) + 1
        # the second and the last pair are the same alignment: neither its place nor its company changes it
        assert bc.same_result(want[1][0], want[6][0]) == []
    finally:
        for t in (target, nothing, index):
            t.close()


# ---- sharing ----------------------------------------------------------------------------------------------------------------------------
def test_pairs_share_a_target_and_a_source(dl, ctx):
    scene = bc.zoo_targets()["scene"]
    o = options_of(dl, nd.STEP_MORE_THUENTE, maximum_iterations=1)
    target, other, index = dl.NdtTarget(ctx, scene, o), dl.NdtTarget(ctx, scene[:1500], o), dl.NnIndex(ctx, scene)
    sources = [(scene[s::3] + np.float32([0.05 * s, -0.04, 0.02])).astype(np.float32) for s in range(4)]
    shared = dl.PointCloud(ctx, sources[0])
    try:
        before = dl.Ndt(target, o, fitness_index=index).align(sources[1], want_aligned=True)
        pairs = [(target, shared, None, index), (target, sources[1], None, index), (other, shared, bc.MOVED_GUESS, None),
                 (target, sources[2], None, None), (target, sources[3], bc.MOVED_GUESS, index), (target, shared, bc.GENERIC_GUESS, index)]
        assert sum(1 for p in pairs if p[0] is target) == 5 and sum(1 for p in pairs if p[1] is shared) == 3
        want = singles(dl, pairs, o)
        check_batch(dl, ctx, pairs, o, want)
        after = dl.Ndt(target, o, fitness_index=index).align(sources[1], want_aligned=True)  # the target is what it was
        assert bc.same_result(after[0], before[0]) == [] and bc.same_bits(after[1], before[1])
        assert bc.same_bits(shared.download(), sources[0])  # and so is the shared source
    finally:
        for t in (shared, target, other, index):
            t.close()


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pairs", [1, 2, 5, 256])
def test_limit_on_pairs_in_flight(dl, ctx, zoo, max_pairs):
    mode = nd.STEP_MORE_THUENTE
    limits = dl.ndt_batch_default_limits(max_pairs_in_flight=max_pairs)
    stats, plain = check_batch(dl, ctx, zoo["pairs"], zoo["options"][mode], zoo["want"][mode], limits)
    stats_equal(stats, expected(zoo["model"][mode], zoo["pairs"], zoo["sizes"], [True] * 17, max_pairs, limits.max_scratch_bytes))
    stats_equal(plain, expected(zoo["model"][mode], zoo["pairs"], zoo["sizes"], [p[3] is not None for p in zoo["pairs"]], max_pairs,
                                limits.max_scratch_bytes))
    rounds = [bc.rounds_of(k, True) for _, k in zoo["model"][mode]]
    if max_pairs == 1:
        assert stats["read_backs"] == sum(rounds) and stats["mixed_steps"] == 0
    if max_pairs >= 17:
        assert stats["read_backs"] == max(rounds)


@pytest.mark.parametrize("cut", ["three_chunks", "before_every_large_pair", "smaller_than_any_pair", "exactly_all"])
def test_limit_on_scratch_bytes(dl, ctx, zoo, cut):
    mode, sizes = nd.STEP_CLAMPED, zoo["sizes"]
    budget = {"three_chunks": sum(sizes) // 3, "before_every_large_pair": max(sizes), "smaller_than_any_pair": min(sizes) - 1,
              "exactly_all": sum(sizes)}[cut]
    limits = dl.ndt_batch_default_limits(max_pairs_in_flight=256, max_scratch_bytes=budget)
    stats, _ = check_batch(dl, ctx, zoo["pairs"], zoo["options"][mode], zoo["want"][mode], limits)
    runs = bc.chunks(sizes, 256, budget)
    print(cut, budget, runs, stats)
    stats_equal(stats, expected(zoo["model"][mode], zoo["pairs"], sizes, [True] * 17, 256, budget))
    if cut in ("three_chunks", "before_every_large_pair"):
        assert len(runs) >= 3
    if cut == "smaller_than_any_pair":
        assert stats["chunks"] == 17 and stats["max_in_flight"] == 1
    if cut == "exactly_all":
        assert stats["chunks"] == 1


# ---- order, determinism, profiling ------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_pairs_permutes_the_results(dl, ctx, zoo):
    mode = nd.STEP_MORE_THUENTE
    order = np.random.RandomState(3).permutation(17)
    pairs, want = [zoo["pairs"][i] for i in order], [zoo["want"][mode][i] for i in order]
    check_batch(dl, ctx, pairs, zoo["options"][mode], want)
    check_batch(dl, ctx, zoo["pairs"][::-1], zoo["options"][mode], zoo["want"][mode][::-1], dl.ndt_batch_default_limits(max_pairs_in_flight=5))


def test_two_calls_give_the_same_bytes(dl, ctx, zoo):
    o = zoo["options"][nd.STEP_MORE_THUENTE]
    a = dl.ndt_align_batch(ctx, zoo["pairs"], o, want_aligned=True)
    b = dl.ndt_align_batch(ctx, zoo["pairs"], o, want_aligned=True)
    assert a[1] == b[1]
    for ra, rb, ca, cb in zip(a[0], b[0], a[2], b[2]):
        assert bc.same_result(ra, rb) == [] and bc.same_bits(ca, cb)


def test_profiled_batch_reports_stage_times(dl, ctx, zoo):
    o, pairs = zoo["options"][nd.STEP_MORE_THUENTE], zoo["pairs"][2:7]
    plain, plain_stats = dl.ndt_align_batch(ctx, pairs, o)
    assert plain_stats["evaluate_ms"] == plain_stats["reduce_ms"] == plain_stats["fitness_ms"] == plain_stats["host_ms"] == 0.0
    ctx.set_profiling(1)
    try:
        timed, stats = dl.ndt_align_batch(ctx, pairs, o)
    finally:
        ctx.set_profiling(0)
    assert stats["evaluate_ms"] > 0 and stats["reduce_ms"] > 0 and stats["fitness_ms"] > 0 and stats["host_ms"] > 0
    assert stats["synchronizations"] == 1
    for a, b in zip(timed, plain):
        assert bc.same_result(a, b) == [] and a["evaluate_ms"] == a["host_ms"] == 0.0


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(dl, ctx, zoo):
    L = ctx._L
    mode = nd.STEP_CLAMPED
    scene = bc.zoo_targets()["scene"]
    other_ctx = dl.Context(0)
    o = zoo["options"][mode]
    foreign_target, foreign_index = dl.NdtTarget(other_ctx, scene, o), dl.NnIndex(other_ctx, scene)
    source = zoo["pairs"][2][1]
    foreign_cloud, cloud = dl.PointCloud(other_ctx, source), dl.PointCloud(ctx, source)
    target, index = zoo["pairs"][2][0], zoo["pairs"][2][3]
    coarse = dl.NdtTarget(ctx, scene, dl.ndt_options(resolution=2.0))
    try:
        def table(entries):
            t = (dl.NdtPair * len(entries))()
            for i, (tg, src, ix, guess) in enumerate(entries):
                t[i].target, t[i].source, t[i].fitness_index = tg, src, ix
                t[i].guess[:] = list(np.float64(guess).reshape(16))
            return t

        eye, scaled, nan = np.eye(4), np.eye(4), np.eye(4)
        scaled[:3, :3] *= 1.001
        nan[0, 3] = np.nan
        good = [(target.h, cloud.h, index.h, zoo["pairs"][2][2])] * 3  # the zoo's pair 2, three times
        lim = dl.ndt_batch_default_limits()

        def call(entries, count=None, options=o, limits=lim, ctx_h=ctx.h, results="own", pairs="own"):
            r = (dl.NdtResult * 4)()
            for k in range(4):
                r[k].iterations = -77  # a sentinel no alignment writes
            t = table(entries)
            before = (ctx.read_backs(), ctx.synchronizations())
            status = L.dliom_ndt_align_batch(ctx_h, t if pairs == "own" else None, len(entries) if count is None else count,
                                             None if options is None else C.byref(options), None if limits is None else C.byref(limits),
                                             r if results == "own" else None, None, None)
            assert (ctx.read_backs(), ctx.synchronizations()) == before or status == dl.OK
            return status, [r[k].iterations for k in range(4)]

        bad = dl.ERR_INVALID_ARGUMENT
        untouched = [-77] * 4
        assert call(good) == (dl.OK, [zoo["want"][mode][2][0]["iterations"]] * 3 + [-77])
        assert call(good, ctx_h=None) == (bad, untouched)
        assert call(good, pairs=None) == (bad, untouched)
        assert call(good, results=None)[0] == bad
        assert call(good, options=None) == (bad, untouched)
        assert call(good, count=-1) == (bad, untouched)
        for wrong in (dict(resolution=0.0), dict(step_size=float("inf")), dict(outlier_ratio=1.0), dict(transformation_epsilon=-1e-9),
                      dict(maximum_iterations=-1), dict(min_points_per_voxel=2), dict(step_mode=2), dict(reserved=1)):
            assert call(good, options=dl.ndt_options(**wrong)) == (bad, untouched), wrong
        for wrong in (dict(max_pairs_in_flight=0), dict(max_pairs_in_flight=257), dict(reserved=1), dict(max_scratch_bytes=0),
                      dict(max_scratch_bytes=-5)):
            assert call(good, limits=dl.ndt_batch_default_limits(**wrong)) == (bad, untouched), wrong
        assert call(good[:2] + [(None, cloud.h, index.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(target.h, None, index.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(foreign_target.h, cloud.h, index.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(target.h, foreign_cloud.h, index.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(target.h, cloud.h, foreign_index.h, eye)]) == (bad, untouched)
        # a bad guess or another resolution in the LAST pair fails the call before the first pair runs
        assert call(good[:2] + [(target.h, cloud.h, index.h, scaled)]) == (bad, untouched)
        assert call(good[:2] + [(target.h, cloud.h, index.h, nan)]) == (bad, untouched)
        assert call(good[:2] + [(coarse.h, cloud.h, index.h, eye)]) == (bad, untouched)
        assert call(good, options=dl.ndt_options(resolution=2.0)) == (bad, untouched)
        # a NULL index is no refusal; count == 0 succeeds and launches nothing; limits NULL are the defaults
        assert call(good[:2] + [(target.h, cloud.h, None, eye)])[0] == dl.OK
        assert call(good, count=0) == (dl.OK, untouched)
        assert call(good, limits=None)[0] == dl.OK
        before = ctx.read_backs()
        results, stats = dl.ndt_align_batch(ctx, [])
        assert results == [] and ctx.read_backs() == before
        assert stats == dict(pairs=0, chunks=0, steps=0, read_backs=0, synchronizations=0, max_in_flight=0, pair_evaluations=0,
                             pair_searches=0, evaluation_launches=[0, 0, 0], mixed_steps=0, evaluate_ms=0.0, reduce_ms=0.0,
                             fitness_ms=0.0, host_ms=0.0)
    finally:
        for t in (coarse, cloud, foreign_cloud, foreign_index, foreign_target):
            t.close()
        other_ctx.close()


# ---- the C++ adapters -------------------------------------------------------------------------------------------------------------------
def test_adapter_program(dl, tmp_path):
    """tests/cpp/ndt_batch_adapter.cc builds with g++ -Wall -Werror and holds: AlignPairsNdt builds one target for a target
    cloud that several pairs name and gives NormalDistributionsTransform's results; GenerateGroundTruthNdt on a 12-node
    trajectory (one `from` node without a revisit, one pair with nothing to align -- which ICP does not converge on; NDT as dliom.h states
    it cannot report non-convergence for finite input -- and stamps past the bag's end) is
    byte-equal to the pair-at-a-time loop through NormalDistributionsTransform::GroundTruthNdt for batch sizes 1, 3 and
    100; GenerateGroundTruthIcp's text is what the pair-at-a-time ICP loop gives."""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path / "ndt_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "ndt_batch_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
