"""The batched loop-closure calls at their limits: every chunk capacity of dliom_fast_csm_match_batch (kChunkTop,
kChunkCellBytes, kChunkScans), each of its single-call fallbacks, a frontier that overflows its output records, matchers
of different depths in one chunk; and dliom_csm3d_match_batch over several launches, with refusals and one-launch
fallbacks mixed in, and with eight clouds.  Each test asserts through the call's dliom_batch_stats that it reached its
limit, and that every batched result equals the single call's; the oracle checks all results where it is cheap and a
fixed sample where it is not (said in the test)."""
import numpy as np
import pytest

from helpers import DEFAULT_CSM, build_oracle_submap, pose_distance, to_device_grid

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
RES = 0.2


def same_result(a, b):  # test_gpu_fast_csm.same_result
    assert a["found"] == b["found"]
    if a["found"]:
        assert np.float32(a["score"]) == np.float32(b["score"])
        assert np.array_equal(np.asarray(a["pose"]), np.asarray(b["pose"]))
        assert np.float32(a["rotational_score"]) == np.float32(b["rotational_score"])
        assert np.float32(a["low_resolution_score"]) == np.float32(b["low_resolution_score"])
    assert a["num_discrete_scans"] == b["num_discrete_scans"]


def single(q):
    m = q["matcher"]
    if q["kind"] == "Match":
        return m.Match(q["global_node_pose"], q["global_submap_pose"], q["data"], q["min_score"])
    if q["kind"] == "MatchFullSubmap":
        return m.MatchFullSubmap(q["global_node_rotation"], q["global_submap_rotation"], q["data"], q["min_score"])
    return m.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"])


def oracle_of(om, q):
    if q["kind"] == "Match":
        return om.Match(q["global_node_pose"], q["global_submap_pose"], q["data"], q["min_score"])
    return om.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"])


def opts(depth, xy, z, ang_deg=5.0, frd=None, min_rot=0.0, min_low=0.2):
    """Windows in cells of RES (lround(window / RES) == xy, z)."""
    return dict(branch_and_bound_depth=depth, full_resolution_depth=frd or depth, min_rotational_score=min_rot,
                min_low_resolution_score=min_low, linear_xy_search_window=RES * xy, linear_z_search_window=RES * z,
                angular_search_window=np.deg2rad(ang_deg))


def lowest(depth, xy, z, scans=1):
    step = 1 << (depth - 1)
    return ((2 * xy + step) // step) ** 2 * ((2 * z + step) // step) * scans


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


class Scene:
    """Corkscrew scans 0-5 in a 0.2 m and a 0.5 m submap; node data of scans along the trajectory."""

    def __init__(self, dl, ctx, orc):
        from dliom import synth
        self.dl, self.ctx, self.orc = dl, ctx, orc
        self.og_hi = build_oracle_submap(orc, RES, num_scans=6, beams=16, azimuths=256, max_range=40.0)
        self.og_lo = build_oracle_submap(orc, 0.5, num_scans=6, beams=16, azimuths=256)
        self.g_hi, self.g_lo = to_device_grid(dl, ctx, self.og_hi), to_device_grid(dl, ctx, self.og_lo)
        self.scans = {}
        self.matchers = []

    def matcher(self, o, hsize=30):
        from dliom import synth
        hists = [self.orc.compute_histogram(synth.scan(synth.trajectory_pose(0.1 * s), 16, 256)[0], hsize) for s in range(6)]
        yaws = [0.02 * s for s in range(6)]
        om = self.orc.FastCorrelativeScanMatcher3D(self.og_hi, self.og_lo, np.array(hists), yaws, o)
        dm = self.dl.FastCorrelativeScanMatcher3D(self.ctx, self.g_hi, self.g_lo, np.array(hists), yaws, o)
        self.matchers.append(dm)
        return om, dm

    def node(self, t, n_hi=150, dense=False, hsize=30):
        """(truth, node data) of the scan at trajectory time t; n_hi points of a 16 x 256 (dense: 32 x 512) scan."""
        from dliom import synth
        key = (round(t, 6), dense)
        if key not in self.scans:
            truth = synth.trajectory_pose(t)
            self.scans[key] = truth, synth.scan(truth, 32, 512)[0] if dense else synth.scan(truth, 16, 256)[0]
        truth, pts = self.scans[key]
        rng = np.random.RandomState(int(1000 * t) + n_hi)
        hi = pts[rng.choice(len(pts), n_hi, replace=n_hi > len(pts))]
        return truth, dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=hi,
                           low_resolution_point_cloud=pts[::7][:120],
                           rotational_scan_matcher_histogram=self.orc.compute_histogram(pts, hsize))


@pytest.fixture(scope="module")
def scene(dl, ctx, orc):
    s = Scene(dl, ctx, orc)
    yield s
    for m in s.matchers:
        m.close()


def q3dof(dm, truth, data, k, min_score):
    g = np.array(truth, dtype=np.float64).copy()
    g[:3] += 0.3 * np.array([np.cos(1.3 * k), np.sin(0.7 * k), 0.2 * np.cos(k)])
    return dict(kind="MatchWith3DofInitial", matcher=dm, pose_in_submap_guess=g, data=data, min_score=min_score)


def qmatch(dm, truth, data, k, min_score):
    from dliom import synth
    return dict(kind="Match", matcher=dm, global_node_pose=synth.perturb_pose(truth, 0.2, 1.0, seed=k),
                global_submap_pose=IDENT, data=data, min_score=min_score)


def check_against_single(dl, ctx, qs):
    results, statuses, stats = dl.fast_csm_match_batch(ctx, qs)
    assert statuses == [0] * len(qs)
    assert stats["batched"] + stats["per_query"] + stats["without_search"] == len(qs)
    for q, r in zip(qs, results):
        same_result(r, single(q))
    return results, stats


# ---- fast search: the three capacities that close a chunk before kChunkSearches ----------------------------------
def test_chunk_split_on_lowest_candidates(dl, ctx, scene):
    """kChunkTop (2^18): 100 3-DoF searches of 2 925 and 3 328 lowest-resolution candidates each (~313 000 in all)
    need two chunks where kChunkSearches alone needs one.  Every result equals the single call's, in query order; the
    oracle checks every tenth (an exhaustive search here is 2e4 candidates)."""
    oms, dms = zip(*[scene.matcher(opts(2, 14, 12)), scene.matcher(opts(2, 15, 12, min_low=0.1))])
    assert lowest(2, 14, 12) == 2925 and lowest(2, 15, 12) == 3328
    qs, owner = [], []
    for k in range(100):
        truth, data = scene.node(0.05 * (k % 10) + 0.1)
        j = (k // 3) % 2
        qs.append(q3dof(dms[j], truth, data, k, (0.25, 0.4, 0.55)[k % 3]))
        owner.append(j)
    results, stats = check_against_single(dl, ctx, qs)
    assert stats["batched"] == 100 and stats["per_query"] == 0
    assert stats["chunks"] == 2 > int(np.ceil(100 / 128)) and stats["frontier_chains"] == 2
    assert any(r["found"] for r in results)
    for k in range(0, 100, 10):
        same_result(results[k], oracle_of(oms[owner[k]], qs[k]))


def test_chunk_split_on_cell_bytes(dl, ctx, scene):
    """kChunkCellBytes (256 MB): 12 Match searches of 8 000 points, one of them 60 m out, over ~420 discrete scans each
    (~40 MB of cells each) need two chunks or more.  Every result equals the single call's; the oracle checks two (an
    exhaustive search here is 3e7 lookups)."""
    om, dm = scene.matcher(opts(2, 1, 0, ang_deg=40.0))
    qs = []
    for k in range(12):
        truth, data = scene.node(0.1 + 0.04 * k, n_hi=8000, dense=True)
        hi = data["high_resolution_point_cloud"].copy()
        hi[k] = hi[k] / np.linalg.norm(hi[k]) * 60.0
        qs.append(qmatch(dm, truth, dict(data, high_resolution_point_cloud=hi), k, (0.3, 0.5)[k % 2]))
    results, stats = check_against_single(dl, ctx, qs)
    cells = sum(3 * r["num_discrete_scans"] * 8000 * 4 for r in results)
    assert cells > 256 << 20 and all(r["num_discrete_scans"] * lowest(2, 1, 0) <= 4096 for r in results)
    assert stats["batched"] == 12 and stats["chunks"] >= 2 > int(np.ceil(12 / 128))
    for k in (0, 7):
        same_result(results[k], oracle_of(om, qs[k]))


def test_chunk_split_on_discrete_scans(dl, ctx, scene):
    """kChunkScans (65 535): 70 Match searches of 40 points, one of them 200 m out, so that the angular step is ~1 mrad
    and a 0.6 rad window makes ~1 200 discrete scans (all kept: min_rotational_score 0) of one lowest-resolution
    candidate each (zero linear windows).  Every result equals the single call's and the oracle's, in query order."""
    om, dm = scene.matcher(opts(3, 0, 0, ang_deg=34.0))
    qs = []
    for k in range(70):
        truth, data = scene.node(0.1 + 0.01 * k, n_hi=40)
        hi = data["high_resolution_point_cloud"].copy()
        hi[k % 40] = hi[k % 40] / np.linalg.norm(hi[k % 40]) * (200.0 + k)
        qs.append(qmatch(dm, truth, dict(data, high_resolution_point_cloud=hi), k, (0.2, 0.45)[k % 2]))
    results, stats = check_against_single(dl, ctx, qs)
    scans = [r["num_discrete_scans"] for r in results]
    assert min(scans) > 1000 and sum(scans) > 65535
    assert stats["batched"] == 70 and stats["chunks"] >= 2 > int(np.ceil(70 / 128))
    for q, r in zip(qs, results):
        same_result(r, oracle_of(om, q))


def test_frontier_arguments_are_per_search(dl, ctx, scene):
    """Two searches on the same node differing only in min_score (0.9, 0.2): each one's chain runs on its own
    FrontierArgs, so a batch of both fetches on demand exactly what the two batches of one fetch (cache_misses), in
    either order.  Their results cannot show it: a frontier run on another search's min_score changes only what the
    recursion must fetch later.  Both frontiers stay far below kBatchCap and kBatchOutRecords, so the counts are exact."""
    _, dm = scene.matcher(opts(3, 5, 3))
    truth, data = scene.node(0.26)
    hi, lo = q3dof(dm, truth, data, 4, 0.9), q3dof(dm, truth, data, 4, 0.2)
    alone = [check_against_single(dl, ctx, [q])[1]["cache_misses"] for q in (hi, lo)]
    assert alone[0] != alone[1]
    for pair, want in (([hi, lo], alone), ([lo, hi], alone[::-1])):
        results, stats = check_against_single(dl, ctx, pair)
        assert stats["batched"] == 2 and stats["chunks"] == 1
        assert stats["cache_misses"] == sum(want), (stats, alone)


# ---- fast search: what the batch hands to the single call ---------------------------------------------------------
@pytest.mark.parametrize("case", ["depth1", "points8193", "lowest4800", "lowest10800"])
def test_single_call_fallbacks(dl, ctx, orc, scene, case):
    """Depth 1, 8 193 points, 4 097-8 192 and more than 8 192 lowest-resolution candidates: the batch runs that search
    through the single call (per_query_frontier) and the rest batched; both equal the single call and the oracle."""
    o, n_hi, dense = {"depth1": (opts(1, 3, 2), 150, False), "points8193": (opts(3, 3, 2), 8193, True),
                      "lowest4800": (opts(2, 19, 11), 60, False), "lowest10800": (opts(2, 29, 11), 60, False)}[case]
    if case.startswith("lowest"):
        assert 4096 < lowest(2, 19, 11) <= 8192 < lowest(2, 29, 11)
    om, dm = scene.matcher(o)
    om2, dm2 = scene.matcher(opts(3, 3, 2))
    truth, data = scene.node(0.22, n_hi=n_hi, dense=dense)
    truth2, data2 = scene.node(0.31)
    qs = [q3dof(dm2, truth2, data2, 1, 0.3), q3dof(dm, truth, data, 2, 0.3), q3dof(dm2, truth2, data2, 3, 0.4)]
    results, stats = check_against_single(dl, ctx, qs)
    assert stats["per_query_frontier"] == 1 and stats["per_query"] == 1 and stats["batched"] == 2
    for q, r, m in zip(qs, results, (om2, om, om2)):
        same_result(r, oracle_of(m, q))


# ---- fast search: a frontier larger than its output records -------------------------------------------------------
def test_frontier_overflow_flat_landscape(dl, ctx, orc):
    """A flat score landscape (one uniform block of occupied cells) with min_score 0.1 and a low-resolution grid that
    fails every leaf: every candidate expands, so the chain's 1 225 depth-1 records (245 per scan, 5 scans) and their
    ~7 600 leaves overflow kBatchOutRecords, more than kBatchLeavesAhead leaves sit at theta, and the recursion, which
    must visit them all, fetches scores on demand (cache_misses).  Batch, single call and oracle agree (nothing found)."""
    hi, lo = orc.HybridGrid(RES), orc.HybridGrid(0.5)
    r = np.arange(-50, 51)
    x, y, z = np.meshgrid(r, r, np.arange(-15, 16), indexing="ij")
    hi.set_values(np.stack([x.ravel(), y.ravel(), z.ravel()], 1), np.full(x.size, 30000))
    r = np.arange(-20, 21)
    x, y, z = np.meshgrid(r, r, np.arange(-6, 7), indexing="ij")
    lo.set_values(np.stack([x.ravel(), y.ravel(), z.ravel()], 1), np.full(x.size, 2))
    g_hi, g_lo = to_device_grid(dl, ctx, hi), to_device_grid(dl, ctx, lo)
    assert lowest(2, 6, 4) == 245
    # max_norm 3 m: an angular window of two steps and a little holds 2 * 2 + 1 = 5 scans
    o = dict(opts(2, 6, 4, min_low=0.5), angular_search_window=2.0 * 0.99 * np.arccos(1 - RES * RES / (2 * 3.0 * 3.0)) + 1e-4)
    hist = np.ones((1, 10), np.float32)
    om = orc.FastCorrelativeScanMatcher3D(hi, lo, hist, [0.0], o)
    dm = dl.FastCorrelativeScanMatcher3D(ctx, g_hi, g_lo, hist, [0.0], o)
    pts = np.random.RandomState(5).uniform([-2, -2, -1], [2, 2, 1], size=(60, 3)).astype(np.float32)
    pts[0] = [3.0, 0.0, 0.0]
    data = dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=pts, low_resolution_point_cloud=pts[::2],
                rotational_scan_matcher_histogram=np.ones(10, np.float32))
    node = np.array([0, 0, 0, 1.0, 0, 0, 0])
    qs = [dict(kind="Match", matcher=dm, global_node_pose=node, global_submap_pose=IDENT, data=data, min_score=0.1),
          dict(kind="MatchWith3DofInitial", matcher=dm, pose_in_submap_guess=node, data=data, min_score=0.1)]
    try:
        results, stats = check_against_single(dl, ctx, qs)
        assert results[0]["num_discrete_scans"] == 5
        assert stats["batched"] == 2 and stats["cache_misses"] > 0
        for q, r in zip(qs, results):
            assert not r["found"]
            same_result(r, oracle_of(om, q))
    finally:
        dm.close()
        g_hi.close()
        g_lo.close()


def test_mixed_matchers_in_one_chunk(dl, ctx, orc):
    """Three matchers on submaps of 0.15 / 0.2 / 0.3 m with depths 3 / 5 / 7 (so the chain's deepest level is not every
    search's), histogram sizes 10 / 30 / 120, both Match and 3-DoF queries interleaved: one chunk, every result equal to
    the single call's and the oracle's."""
    from dliom import synth
    made, qs, oms = [], [], []
    for res, depth, hsize, frd in ((0.15, 3, 10, 1), (0.2, 5, 30, 3), (0.3, 7, 120, 7)):
        og_hi = build_oracle_submap(orc, res, num_scans=4, beams=16, azimuths=256, max_range=30.0)
        og_lo = build_oracle_submap(orc, 0.5, num_scans=4, beams=16, azimuths=256)
        g_hi, g_lo = to_device_grid(dl, ctx, og_hi), to_device_grid(dl, ctx, og_lo)
        hists = [orc.compute_histogram(synth.scan(synth.trajectory_pose(0.1 * s), 16, 256)[0], hsize) for s in range(4)]
        o = dict(branch_and_bound_depth=depth, full_resolution_depth=frd, min_rotational_score=0.2,
                 min_low_resolution_score=0.2, linear_xy_search_window=1.2, linear_z_search_window=0.6,
                 angular_search_window=np.deg2rad(3.0))
        om = orc.FastCorrelativeScanMatcher3D(og_hi, og_lo, np.array(hists), [0.0] * 4, o)
        dm = dl.FastCorrelativeScanMatcher3D(ctx, g_hi, g_lo, np.array(hists), [0.0] * 4, o)
        made += [dm, g_hi, g_lo]
        oms.append((om, og_hi, og_lo))
        for k in range(4):
            truth = synth.trajectory_pose(0.07 * k + 0.05)
            pts, _ = synth.scan(truth, 16, 256)
            data = dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=pts[::(17 + k)],
                        low_resolution_point_cloud=pts[::31], rotational_scan_matcher_histogram=orc.compute_histogram(pts, hsize))
            mk = qmatch if k % 2 else q3dof
            qs.append((len(oms) - 1, mk(dm, truth, data, 10 * depth + k, (0.3, 0.45, 0.35, 0.6)[k])))
    order = np.random.RandomState(3).permutation(len(qs))
    qs = [qs[i] for i in order]
    try:
        results, stats = check_against_single(dl, ctx, [q for _, q in qs])
        assert stats["chunks"] == 1 and stats["batched"] == len(qs) and stats["per_query"] == 0
        assert any(r["found"] for r in results)
        for (j, q), r in zip(qs, results):
            same_result(r, oracle_of(oms[j][0], q))
    finally:
        for h in made:
            h.close()


# ---- the LM batch -----------------------------------------------------------------------------------------------
def lm_problems(scene, count, seed):
    """count problems on the scene's grids: perturbed truths of scans along the trajectory, high / low clouds."""
    from dliom import synth
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        truth, data = scene.node(0.05 * (k % 12) + 0.1, n_hi=int(rng.randint(60, 200)))
        init = synth.perturb_pose(truth, 0.15, 2.0, seed=seed + k)
        out.append((init[:3] + rng.uniform(-0.05, 0.05, 3), init,
                    [(data["high_resolution_point_cloud"], scene.g_hi, scene.og_hi),
                     (data["low_resolution_point_cloud"], scene.g_lo, scene.og_lo)]))
    return out


def as_device(p):
    return p[0], p[1], [(c, g) for c, g, _ in p[2]]


def check_oracle(orc, copts, p, pose, summary):
    ro = orc.csm3d_match(copts, p[0], p[1], [(c, og) for c, _, og in p[2]])
    dt, dr = pose_distance(pose, ro["pose"])
    assert dt <= 1e-6 and dr <= 1e-6
    assert summary["num_iterations"] == ro["num_iterations"]


def test_lm_batch_three_launches(dl, ctx, orc, scene):
    """600 problems: three launches of csm_lm_batch_kernel (kChunk 256).  Each pose and summary equals Match() bit for
    bit, in any order (the batch again on a shuffled list); the oracle checks every 20th (600 CPU solves would dominate)."""
    copts = dict(DEFAULT_CSM, use_nonmonotonic_steps=True)
    csm = dl.CeresScanMatcher3D(ctx, copts)
    probs = lm_problems(scene, 600, 700)
    poses, summaries, statuses, stats = csm.match_batch([as_device(p) for p in probs])
    assert statuses == [0] * 600
    assert stats["lm_launches"] == 3 and stats["chunks"] == 3 and stats["batched"] == 600
    for k, p in enumerate(probs):
        p1, s1 = csm.Match(*as_device(p))
        assert np.array_equal(poses[k], p1) and summaries[k] == s1, k
        if k % 20 == 0:
            check_oracle(orc, copts, p, poses[k], summaries[k])
    perm = np.random.RandomState(11).permutation(600)
    poses2, summaries2, statuses2, stats2 = csm.match_batch([as_device(probs[i]) for i in perm])
    assert statuses2 == [0] * 600 and stats2["lm_launches"] == 3
    for j, i in enumerate(perm):
        assert np.array_equal(poses2[j], poses[i]) and summaries2[j] == summaries[i]


def test_lm_batch_mixed_outcomes(dl, ctx, orc, scene):
    """In one batch with solved problems: no cloud and a cloud count the options' weights do not match (ERR_WEIGHTS),
    an empty host cloud (ERR_EMPTY_CLOUD), and problems above a lowered DLIOM_TUNE_CSM_ONE_LAUNCH_MAX (the single call's
    path).  Every status, pose and summary equals the single call's; a refused problem's pose and summary are zeros."""
    copts = dict(DEFAULT_CSM, max_num_iterations=2)
    csm = dl.CeresScanMatcher3D(ctx, copts)
    base = lm_problems(scene, 10, 900)
    probs = [as_device(p) for p in base]
    hi = base[0][2][0]
    probs.insert(2, (base[0][0], base[0][1], []))
    probs.insert(5, (base[1][0], base[1][1], [(hi[0], hi[1]), (base[1][2][1][0], scene.g_lo), (hi[0][:5], scene.g_lo)]))
    probs.insert(7, (base[2][0], base[2][1], [(hi[0], hi[1]), (np.zeros((0, 3), np.float32), scene.g_lo)]))
    refused = {2: dl.ERR_WEIGHTS, 5: dl.ERR_WEIGHTS, 7: dl.ERR_EMPTY_CLOUD}
    keep = ctx.get_tuning(dl.TUNE_CSM_ONE_LAUNCH_MAX)
    ctx.set_tuning(dl.TUNE_CSM_ONE_LAUNCH_MAX, 250)
    try:
        poses, summaries, statuses, stats = csm.match_batch(probs)
        big = [k for k, p in enumerate(probs) if k not in refused and sum(len(c) for c, _ in p[2]) > 250]
        assert stats["per_query_one_launch"] == len(big) > 0 and stats["without_search"] == 3
        assert stats["batched"] == len(probs) - 3 - len(big) > 0 and stats["lm_launches"] == 1
        for k, p in enumerate(probs):
            if k in refused:
                assert statuses[k] == refused[k]
                with pytest.raises(dl.DliomError) as e:
                    csm.Match(*p)
                assert e.value.status == refused[k]
                assert not poses[k].any() and all(v == 0 for v in summaries[k].values())
                continue
            assert statuses[k] == 0
            p1, s1 = csm.Match(*p)
            assert np.array_equal(poses[k], p1) and summaries[k] == s1, k
    finally:
        ctx.set_tuning(dl.TUNE_CSM_ONE_LAUNCH_MAX, keep)
    assert ctx.get_tuning(dl.TUNE_CSM_ONE_LAUNCH_MAX) == keep
    for k, b in zip([k for k in range(len(probs)) if k not in refused], base):
        check_oracle(orc, copts, b, poses[k], summaries[k])


def test_lm_batch_eight_clouds(dl, ctx, orc, scene):
    """DLIOM_MAX_CLOUDS (8) clouds on one problem, twice in one batch: four device clouds and four host arrays on both
    grids; equal to Match() bit for bit and to the oracle."""
    from dliom import synth
    copts = dict(DEFAULT_CSM, occupied_space_weight=[1.0, 6.0, 0.5, 2.0, 3.0, 1.5, 4.0, 0.75])
    csm = dl.CeresScanMatcher3D(ctx, copts)
    truth, data = scene.node(0.27, n_hi=200)
    pts = data["high_resolution_point_cloud"]
    clouds = [(pts[k::8] if k % 2 else pts[k::3], (scene.g_hi, scene.og_hi) if k % 3 else (scene.g_lo, scene.og_lo))
              for k in range(8)]
    init = synth.perturb_pose(truth, 0.1, 1.5, seed=8)
    dev = [dl.PointCloud(ctx, c) for c, _ in clouds[:4]]
    try:
        prob = (init[:3], init, [(d, g[0]) for d, (_, g) in zip(dev, clouds[:4])] + [(c, g[0]) for c, g in clouds[4:]])
        poses, summaries, statuses, stats = csm.match_batch([prob, prob])
        assert statuses == [0, 0] and stats["batched"] == 2
        p1, s1 = csm.Match(init[:3], init, [(c, g[0]) for c, g in clouds])
        for k in range(2):
            assert np.array_equal(poses[k], p1) and summaries[k] == s1
        ro = orc.csm3d_match(copts, init[:3], init, [(c, g[1]) for c, g in clouds])
        dt, dr = pose_distance(poses[0], ro["pose"])
        assert dt <= 1e-6 and dr <= 1e-6 and summaries[0]["num_iterations"] == ro["num_iterations"]
    finally:
        for d in dev:
            d.close()
