"""dliom_icp_align_batch on the device: every pair's result and aligned cloud equal dliom_icp_align's bits, whatever the
chunking, the order and the company of a pair, and the call's statistics are those of the fixed schedule (dliom.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_batch_common as bc  # noqa: E402
import icp_common as ic  # noqa: E402

pytestmark = pytest.mark.gpu

SOURCE_SIZES = (0, 1, 65, 2047, 2048, 2049, 4097)  # the tree's workgroup boundary, and an empty source
TARGET_SIZES = (1, 65, 1025, 4097)  # 1 to 17 brute-force segments in one launch


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


def options_of(dl, **overrides):
    return dl.icp_options(**{k: v for k, v in ic.options(**overrides).items() if k in ic.DEFAULTS})


def small_guess(seed):
    return ic.pose_matrix(ic.synth.perturb_pose(ic.IDENTITY7, 0.05, 0.5, seed=seed))


def singles(dl, pairs, options):
    """dliom_icp_align pair by pair -> [(result, aligned points)]"""
    return [dl.Icp(index, options).align(source, guess, want_aligned=True) for index, source, guess in pairs]


def check_batch(dl, ctx, pairs, options, want, limits=None):
    """One batched call whose results and clouds equal `want` (singles' output) -> its statistics"""
    before = ctx.read_backs()
    results, stats, clouds = dl.icp_align_batch(ctx, pairs, options, limits, want_aligned=True)
    assert ctx.read_backs() - before == stats["read_backs"] == stats["steps"]
    assert len(results) == len(clouds) == len(want) == stats["pairs"]
    for i, ((single, points), got, cloud) in enumerate(zip(want, results, clouds)):
        assert bc.same_result(got, single) == [], (i, bc.same_result(got, single), got, single)
        assert bc.same_bits(cloud, points), i
        assert got["search_ms"] == got["reduce_ms"] == got["solve_ms"] == got["transform_ms"] == 0.0
    assert stats["pair_searches"] == sum(r["read_backs"] for r, _ in want)
    plain, plain_stats = dl.icp_align_batch(ctx, pairs, options, limits)  # without the clouds: the same results
    assert all(bc.same_result(a, b) == [] for a, b in zip(plain, results))
    assert plain_stats["synchronizations"] == 0 and stats["synchronizations"] == stats["chunks"]
    return stats


# ---- the zoo: 17 pairs over every source and target size ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo(dl, ctx):
    rng = np.random.RandomState(17)
    base = bc.cloud_points(rng, 4097)
    targets = {n: base[:n].copy() for n in TARGET_SIZES}
    indices = {n: dl.NnIndex(ctx, t) for n, t in targets.items()}
    arrays, pairs = [], []
    for i in range(17):
        ns, nt = SOURCE_SIZES[i % len(SOURCE_SIZES)], TARGET_SIZES[(i + i // 7) % len(TARGET_SIZES)]
        motion = ic.synth.perturb_pose(ic.IDENTITY7, 0.2, 1.5, seed=40 + i)
        picked = base[rng.permutation(4097)[:ns]] + (0.02 * rng.standard_normal((ns, 3))).astype(np.float32)
        source = ic.synth.transform_points(motion, picked).astype(np.float32).reshape(-1, 3)
        guess = None if i % 2 == 0 else small_guess(i)
        arrays.append((source, targets[nt], guess))
        pairs.append((indices[nt], source, guess))
    assert {len(s) for s, _, _ in arrays} == set(SOURCE_SIZES) and {len(t) for _, t, _ in arrays} == set(TARGET_SIZES)
    options = options_of(dl, maximum_iterations=8)
    want = singles(dl, pairs, options)
    yield dict(pairs=pairs, arrays=arrays, options=options, want=want)
    for index in indices.values():
        index.close()


@pytest.mark.parametrize("count", [1, 2, 3, 17])
def test_batch_equals_singles(dl, ctx, zoo, count):
    first = {1: 4, 2: 2, 3: 0, 17: 0}[count]  # K = 1 and 2 start at pairs with points; 3 and 17 begin with the empty source
    pairs, want = zoo["pairs"][first:first + count], zoo["want"][first:first + count]
    stats = check_batch(dl, ctx, pairs, zoo["options"], want, dl.icp_batch_default_limits(max_pairs_in_flight=256))
    searches = [r["read_backs"] for r, _ in want]
    print("K", count, "searches", searches, "stats", stats)
    assert stats["chunks"] == 1 and stats["max_in_flight"] == count
    assert stats["steps"] == stats["read_backs"] == max(searches)  # not their sum: what the call exists for
    if count == 17:
        assert len(set(searches)) > 1 and stats["read_backs"] < sum(searches)


def test_four_pairs_equal_the_cpu_model(dl, ctx, zoo):
    """Pairs 2, 3, 5 and 8 (65 x 1025, 2047 x 4097, 2049 x 65, 1 x 65 points) against tests/icp_common.py"""
    chosen = [2, 3, 5, 8]
    results, _, clouds = dl.icp_align_batch(ctx, [zoo["pairs"][i] for i in chosen], zoo["options"], want_aligned=True)
    for i, got, cloud in zip(chosen, results, clouds):
        source, target, guess = zoo["arrays"][i]
        want = ic.align(source, target, guess, ic.options(maximum_iterations=8))
        for name in ("converged", "reason", "iterations", "correspondences", "fitness_count"):
            assert got[name] == want[name], (i, name, got[name], want[name])
        for name in ("mse", "fitness_score", "transform"):
            assert bc.same_bits(np.float64(got[name]).reshape(-1), np.float64(want[name]).reshape(-1)), (i, name)
        assert bc.same_bits(cloud, want["aligned"]), i


# ---- pairs that end at different steps ------------------------------------------------------------------------------------------------
def test_pairs_that_end_at_different_steps(dl, ctx):
    rng = np.random.RandomState(23)
    scene = bc.cloud_points(rng, 1500)
    moved = ic.synth.transform_points(ic.synth.perturb_pose(ic.IDENTITY7, 0.3, 2.0, seed=5), scene[::2]).astype(np.float32)
    far = scene[:300] + np.float32([500.0, 0.0, 0.0])  # nothing within 3 m: fewer than min_correspondences at k = 1
    holes = moved.copy()
    holes[::9, 0] = np.nan
    holes[4::13, 2] = -np.inf
    index, nothing = dl.NnIndex(ctx, scene), dl.NnIndex(ctx, np.full((40, 3), np.nan, np.float32))
    try:
        pairs = [(index, moved, None), (index, scene, None), (index, moved, small_guess(3)), (index, far, None),
                 (nothing, moved, None), (index, holes, None), (index, moved, None)]
        options = options_of(dl, max_correspondence_distance=3.0, maximum_iterations=3)
        want = singles(dl, pairs, options)
        reasons = [r["reason"] for r, _ in want]
        print("reasons", reasons, "searches", [r["read_backs"] for r, _ in want])
        assert want[1][0]["reason"] == dl.ICP_TRANSFORM and want[1][0]["iterations"] == 1  # identical clouds: at once
        assert want[0][0]["reason"] == dl.ICP_ITERATIONS and want[0][0]["iterations"] == 3  # stopped by the count
        assert (want[3][0]["reason"], want[3][0]["iterations"], want[3][0]["read_backs"]) == (dl.ICP_NO_CORRESPONDENCES, 0, 2)
        assert want[3][0]["fitness_count"] == 300  # it still gets its fitness step
        assert want[4][0]["reason"] == dl.ICP_NO_CORRESPONDENCES and want[4][0]["fitness_count"] == 0
        assert np.isnan(want[4][0]["fitness_score"])
        assert want[5][0]["fitness_count"] == int(np.isfinite(holes).all(axis=1).sum())
        assert {2, 4} <= {r["read_backs"] for r, _ in want}  # some pairs leave the list two steps before the others
        stats = check_batch(dl, ctx, pairs, options, want)
        assert stats["chunks"] == 1 and stats["steps"] == max(r["read_backs"] for r, _ in want) == 4
        # the first and the last pair are the same alignment: neither its place nor its company changes it
        assert bc.same_result(want[0][0], want[6][0]) == []
    finally:
        index.close()
        nothing.close()


# ---- sharing ----------------------------------------------------------------------------------------------------------------------------
def test_pairs_share_an_index_and_a_source(dl, ctx):
    rng = np.random.RandomState(31)
    scene = bc.cloud_points(rng, 2049)
    index, other = dl.NnIndex(ctx, scene), dl.NnIndex(ctx, scene[:700])
    options = options_of(dl, maximum_iterations=6)
    sources = [ic.synth.transform_points(ic.synth.perturb_pose(ic.IDENTITY7, 0.2, 1.0, seed=s), scene[s::3]).astype(np.float32)
               for s in range(4)]
    shared = dl.PointCloud(ctx, sources[0])
    try:
        before = dl.Icp(index, options).align(sources[1], want_aligned=True)
        pairs = [(index, shared, None), (index, sources[1], None), (other, shared, small_guess(2)), (index, sources[2], None),
                 (index, sources[3], small_guess(4)), (index, shared, small_guess(6))]
        assert sum(1 for i, _, _ in pairs if i is index) == 5 and sum(1 for _, s, _ in pairs if s is shared) == 3
        want = singles(dl, pairs, options)
        check_batch(dl, ctx, pairs, options, want)
        after = dl.Icp(index, options).align(sources[1], want_aligned=True)  # the index is what it was
        assert bc.same_result(after[0], before[0]) == [] and bc.same_bits(after[1], before[1])
        assert bc.same_bits(shared.download(), sources[0])  # and so is the shared source
    finally:
        shared.close()
        index.close()
        other.close()


# ---- both search paths ------------------------------------------------------------------------------------------------------------------
def test_both_search_paths_in_one_batch(dl, ctx):
    rng = np.random.RandomState(9)
    a = rng.uniform(-1.0, 1.0, (600, 3)).astype(np.float32)
    b = (rng.uniform(-1.0, 1.0, (600, 3)) + [40.0, 0.0, 0.0]).astype(np.float32)
    clusters = np.concatenate([a, b])
    x = np.linspace(-1.0, 41.0, 500)
    between = np.stack([x, rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 500)], axis=1).astype(np.float32)
    scene = bc.cloud_points(rng, 4097)
    moved = ic.synth.transform_points(ic.synth.perturb_pose(ic.IDENTITY7, 0.2, 1.0, seed=8), scene[::2]).astype(np.float32)
    grid, brute = dl.NnIndex(ctx, scene), dl.NnIndex(ctx, scene, search=dl.NN_BRUTE_FORCE)
    two = dl.NnIndex(ctx, clusters, cell_edge=0.5)
    try:
        pairs = [(grid, moved, None), (two, between, None), (brute, moved, None), (brute, between, small_guess(1)),
                 (grid, moved[:65], small_guess(2))]
        options = options_of(dl, maximum_iterations=4)
        want = singles(dl, pairs, options)
        assert want[1][0]["settled_by_brute_force"] > 0 and want[1][0]["settled_by_grid"] > 0  # the walk lists, the scan settles
        assert want[0][0]["settled_by_brute_force"] == 0 and want[2][0]["settled_by_grid"] == 0  # each index's own mode
        assert bc.same_result({**want[0][0], "settled_by_grid": 0, "settled_by_brute_force": 0},
                              {**want[2][0], "settled_by_grid": 0, "settled_by_brute_force": 0}) == []  # the search is exact
        check_batch(dl, ctx, pairs, options, want)
        forced = options_of(dl, maximum_iterations=4)
        forced.search = dl.NN_BRUTE_FORCE
        want = singles(dl, pairs, forced)
        assert all(r["settled_by_grid"] == 0 for r, _ in want)
        check_batch(dl, ctx, pairs, forced, want)
    finally:
        for index in (grid, brute, two):
            index.close()


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pairs", [1, 2, 3, 16, 256])
def test_limit_on_pairs_in_flight(dl, ctx, zoo, max_pairs):
    sizes = [dl.icp_batch_scratch_bytes(len(s)) for s, _, _ in zoo["arrays"]]
    searches = [r["read_backs"] for r, _ in zoo["want"]]
    limits = dl.icp_batch_default_limits(max_pairs_in_flight=max_pairs)
    stats = check_batch(dl, ctx, zoo["pairs"], zoo["options"], zoo["want"], limits)
    want = bc.expected_stats(searches, sizes, max_pairs, limits.max_scratch_bytes)
    assert {k: stats[k] for k in want} == want
    if max_pairs == 1:
        assert stats["read_backs"] == sum(searches)
    if max_pairs >= 17:
        assert stats["read_backs"] == max(searches)


@pytest.mark.parametrize("cut", ["before_pair_5", "before_every_large_pair", "smaller_than_any_pair", "exactly_all"])
def test_limit_on_scratch_bytes(dl, ctx, zoo, cut):
    sizes = [dl.icp_batch_scratch_bytes(len(s)) for s, _, _ in zoo["arrays"]]
    searches = [r["read_backs"] for r, _ in zoo["want"]]
    budget = {"before_pair_5": sum(sizes[:5]) + sizes[5] - 1, "before_every_large_pair": max(sizes), "smaller_than_any_pair": min(sizes) - 1,
              "exactly_all": sum(sizes)}[cut]
    limits = dl.icp_batch_default_limits(max_pairs_in_flight=256, max_scratch_bytes=budget)
    stats = check_batch(dl, ctx, zoo["pairs"], zoo["options"], zoo["want"], limits)
    want = bc.expected_stats(searches, sizes, 256, budget)
    print(cut, budget, bc.chunks(sizes, 256, budget), stats)
    assert {k: stats[k] for k in want} == want
    runs = bc.chunks(sizes, 256, budget)
    if cut == "before_pair_5":
        assert runs[0] == (0, 5)
    if cut == "smaller_than_any_pair":
        assert stats["chunks"] == 17 and stats["max_in_flight"] == 1
    if cut == "exactly_all":
        assert stats["chunks"] == 1


# ---- order, determinism, profiling ------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_pairs_permutes_the_results(dl, ctx, zoo):
    order = np.random.RandomState(3).permutation(17)
    pairs, want = [zoo["pairs"][i] for i in order], [zoo["want"][i] for i in order]
    check_batch(dl, ctx, pairs, zoo["options"], want)
    check_batch(dl, ctx, pairs[::-1], zoo["options"], want[::-1], dl.icp_batch_default_limits(max_pairs_in_flight=5))


def test_two_calls_give_the_same_bytes(dl, ctx, zoo):
    a = dl.icp_align_batch(ctx, zoo["pairs"], zoo["options"], want_aligned=True)
    b = dl.icp_align_batch(ctx, zoo["pairs"], zoo["options"], want_aligned=True)
    assert a[1] == b[1]
    for ra, rb, ca, cb in zip(a[0], b[0], a[2], b[2]):
        assert bc.same_result(ra, rb) == [] and bc.same_bits(ca, cb)


def test_profiled_batch_reports_stage_times(dl, ctx, zoo):
    plain, plain_stats = dl.icp_align_batch(ctx, zoo["pairs"][:5], zoo["options"])
    assert plain_stats["search_ms"] == plain_stats["reduce_ms"] == plain_stats["solve_ms"] == plain_stats["transform_ms"] == 0.0
    dl._check(ctx._L.dliom_ctx_set_profiling(ctx.h, 1), "set_profiling")
    try:
        timed, stats = dl.icp_align_batch(ctx, zoo["pairs"][:5], zoo["options"])
    finally:
        dl._check(ctx._L.dliom_ctx_set_profiling(ctx.h, 0), "set_profiling")
    assert stats["search_ms"] > 0 and stats["reduce_ms"] > 0 and stats["transform_ms"] > 0 and stats["solve_ms"] > 0
    assert stats["synchronizations"] == 1
    for a, b in zip(timed, plain):
        assert bc.same_result(a, b) == [] and a["search_ms"] == a["solve_ms"] == 0.0


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(dl, ctx, zoo):
    L = ctx._L
    other_ctx = dl.Context(0)
    foreign_index = dl.NnIndex(other_ctx, zoo["arrays"][2][1])
    foreign_cloud, cloud = dl.PointCloud(other_ctx, zoo["arrays"][2][0]), dl.PointCloud(ctx, zoo["arrays"][2][0])
    index = zoo["pairs"][2][0]
    try:
        def table(entries):
            t = (dl.IcpPair * len(entries))()
            for i, (ix, src, guess) in enumerate(entries):
                t[i].index, t[i].source = ix, src
                t[i].guess[:] = list(np.float64(guess).reshape(16))
            return t

        eye, scaled, nan = np.eye(4), np.eye(4), np.eye(4)
        scaled[:3, :3] *= 1.001
        nan[0, 3] = np.nan
        good = [(index.h, cloud.h, eye)] * 3
        o, lim = zoo["options"], dl.icp_batch_default_limits()

        def call(entries, count=None, options=o, limits=lim, ctx_h=ctx.h, results="own", pairs="own"):
            r = (dl.IcpResult * 4)()
            for k in range(4):
                r[k].iterations = -77  # a sentinel no alignment writes
            t = table(entries)
            before = (ctx.read_backs(), ctx.synchronizations())
            status = L.dliom_icp_align_batch(ctx_h, t if pairs == "own" else None, len(entries) if count is None else count,
                                             None if options is None else C.byref(options), None if limits is None else C.byref(limits),
                                             r if results == "own" else None, None, None)
            assert (ctx.read_backs(), ctx.synchronizations()) == before or status == dl.OK
            return status, [r[k].iterations for k in range(4)]

        bad = dl.ERR_INVALID_ARGUMENT
        untouched = [-77] * 4
        assert call(good) == (dl.OK, [zoo["want"][2][0]["iterations"]] * 3 + [-77])
        assert call(good, ctx_h=None) == (bad, untouched)
        assert call(good, pairs=None) == (bad, untouched)
        assert call(good, results=None)[0] == bad
        assert call(good, options=None) == (bad, untouched)
        assert call(good, count=-1) == (bad, untouched)
        for wrong in (dict(maximum_iterations=-1), dict(min_correspondences=2), dict(max_correspondence_distance=float("nan")),
                      dict(search=7), dict(reserved=1)):
            assert call(good, options=dl.icp_options(**wrong)) == (bad, untouched), wrong
        for wrong in (dict(max_pairs_in_flight=0), dict(max_pairs_in_flight=257), dict(reserved=1), dict(max_scratch_bytes=0),
                      dict(max_scratch_bytes=-5)):
            assert call(good, limits=dl.icp_batch_default_limits(**wrong)) == (bad, untouched), wrong
        assert call(good[:2] + [(None, cloud.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(index.h, None, eye)]) == (bad, untouched)
        assert call(good[:2] + [(foreign_index.h, cloud.h, eye)]) == (bad, untouched)
        assert call(good[:2] + [(index.h, foreign_cloud.h, eye)]) == (bad, untouched)
        # a bad guess in the LAST pair fails the call before the first pair runs
        assert call(good[:2] + [(index.h, cloud.h, scaled)]) == (bad, untouched)
        assert call(good[:2] + [(index.h, cloud.h, nan)]) == (bad, untouched)
        # count == 0 succeeds and launches nothing; limits NULL are the defaults
        assert call(good, count=0) == (dl.OK, untouched)
        assert call(good, limits=None)[0] == dl.OK
        before = ctx.read_backs()
        results, stats = dl.icp_align_batch(ctx, [])
        assert results == [] and ctx.read_backs() == before
        assert stats == dict(pairs=0, chunks=0, steps=0, read_backs=0, synchronizations=0, pair_searches=0, max_in_flight=0,
                             search_ms=0.0, reduce_ms=0.0, solve_ms=0.0, transform_ms=0.0)
    finally:
        cloud.close()
        foreign_cloud.close()
        foreign_index.close()
        other_ctx.close()


# ---- the C++ adapters -------------------------------------------------------------------------------------------------------------------
def test_adapter_program(dl, tmp_path):
    """tests/cpp/icp_batch_adapter.cc builds with g++ -Wall -Werror and holds: AlignPairs builds one index for a target that
    several pairs share and gives IterativeClosestPoint's results; GenerateGroundTruthIcp on a 12-node trajectory (one
    `from` node without a revisit, one pair that does not converge, one stamp past the bag's end) is byte-equal to the
    pair-at-a-time loop through IterativeClosestPoint::GroundTruthIcp."""
    libdir = os.path.join(ic.ROOT, "d-liom_amd")
    exe = str(tmp_path / "icp_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ic.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ic.ROOT, "tests", "cpp", "icp_batch_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
