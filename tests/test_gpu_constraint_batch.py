"""Batched loop-closure constraints (dliom_fast_csm_match_batch, dliom_csm3d_match_batch, dliom.compute_constraints):
every batched result equals the single call's and the oracle's, whatever the order and the chunking, and the batch
costs one frontier chain and one LM launch instead of a round trip chain per query."""
import os
import subprocess

import numpy as np
import pytest

from helpers import DEFAULT_CSM, build_oracle_submap, pose_distance, to_device_grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
OPTS = dict(branch_and_bound_depth=6, full_resolution_depth=3, min_rotational_score=0.3, min_low_resolution_score=0.3,
            linear_xy_search_window=3.0, linear_z_search_window=1.0, angular_search_window=np.deg2rad(20.0))
KAT_CLOUD = np.array([[4, 0, 0], [4.5, 0, 0], [5, 0, 0], [5.5, 0, 0], [0, 4, 0], [0, 4.5, 0], [0, 5, 0], [0, 5.5, 0],
                      [0, 0, 4], [0, 0, 4.5], [0, 0, 5], [0, 0, 5.5]], dtype=np.float32)
KAT_OPTS = dict(branch_and_bound_depth=6, full_resolution_depth=6, min_rotational_score=0.1,
                min_low_resolution_score=0.15, linear_xy_search_window=0.8, linear_z_search_window=0.8,
                angular_search_window=0.3)


def same_result(a, b):  # test_gpu_fast_csm.same_result
    assert a["found"] == b["found"]
    if a["found"]:
        assert np.float32(a["score"]) == np.float32(b["score"])
        assert np.array_equal(np.asarray(a["pose"]), np.asarray(b["pose"]))
        assert np.float32(a["rotational_score"]) == np.float32(b["rotational_score"])
        assert np.float32(a["low_resolution_score"]) == np.float32(b["low_resolution_score"])
    assert a["num_discrete_scans"] == b["num_discrete_scans"]


def yaw_of(p):
    return float(np.arctan2(2 * (p[3] * p[6] + p[4] * p[5]), 1 - 2 * (p[5] ** 2 + p[6] ** 2)))


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


class Submap:
    """A synthetic submap (scans first .. first + 5 of the corkscrew) as oracle + device grids and matchers."""

    def __init__(self, dl, ctx, orc, first):
        from dliom import synth
        self.og_hi = build_oracle_submap(orc, 0.2, num_scans=6, beams=16, azimuths=256, max_range=40.0, first_scan=first)
        self.og_lo = build_oracle_submap(orc, 0.5, num_scans=6, beams=16, azimuths=256, first_scan=first)
        self.g_hi, self.g_lo = to_device_grid(dl, ctx, self.og_hi), to_device_grid(dl, ctx, self.og_lo)
        hists, yaws = [], []
        for s in range(first, first + 6):
            pose = synth.trajectory_pose(0.1 * s)
            pts, _ = synth.scan(pose, 16, 256)
            hists.append(orc.compute_histogram(pts, 30))
            yaws.append(yaw_of(pose))
        self.om = orc.FastCorrelativeScanMatcher3D(self.og_hi, self.og_lo, np.array(hists), yaws, OPTS)
        self.dm = dl.FastCorrelativeScanMatcher3D(ctx, self.g_hi, self.g_lo, np.array(hists), yaws, OPTS)


@pytest.fixture(scope="module")
def scene(dl, ctx, orc):
    return [Submap(dl, ctx, orc, first) for first in (0, 3, 6)]


def node_data(orc, t):
    from dliom import synth
    truth = synth.trajectory_pose(t)
    pts, _ = synth.scan(truth, 16, 256)
    return truth, dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=orc.adaptive_voxel_filter(2.0, 150, 15.0, pts),
                       low_resolution_point_cloud=orc.adaptive_voxel_filter(4.0, 200, 60.0, pts),
                       rotational_scan_matcher_histogram=orc.compute_histogram(pts, 30))


def guess_3dof(truth, k):
    g = np.array(truth, dtype=np.float64).copy()
    g[:3] += 0.4 * np.array([np.cos(1.3 * k), np.sin(0.7 * k), 0.1 * np.cos(k)])
    return g


def single(m, q, ctx=None):
    if q["kind"] == "Match":
        return m.Match(q["global_node_pose"], q["global_submap_pose"], q["data"], q["min_score"], ctx=ctx)
    if q["kind"] == "MatchFullSubmap":
        return m.MatchFullSubmap(q["global_node_rotation"], q["global_submap_rotation"], q["data"], q["min_score"], ctx=ctx)
    return m.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"], ctx=ctx)


def oracle_of(om, q):
    if q["kind"] == "Match":
        return om.Match(q["global_node_pose"], q["global_submap_pose"], q["data"], q["min_score"])
    if q["kind"] == "MatchFullSubmap":
        return om.MatchFullSubmap(q["global_node_rotation"], q["global_submap_rotation"], q["data"], q["min_score"])
    return om.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"])


def mixed_queries(orc, scene):
    from dliom import synth
    qs = []
    for si, sm in enumerate(scene):
        truth, data = node_data(orc, 0.1 * (3 * si) + 0.25)
        for k in range(3):
            node = synth.perturb_pose(truth, 1.0 + 0.2 * k, 6.0, seed=40 + 3 * si + k)
            qs.append(dict(kind="Match", sm=si, global_node_pose=node, global_submap_pose=IDENT, data=data,
                           min_score=(0.2, 0.3, 0.45)[k]))
            qs.append(dict(kind="MatchWith3DofInitial", sm=si, pose_in_submap_guess=guess_3dof(truth, k + 5 * si),
                           data=data, min_score=(0.25, 0.35, 0.2)[k]))
        qs.append(dict(kind="MatchWith3DofInitial", sm=si, pose_in_submap_guess=guess_3dof(truth, 1), data=data,
                       min_score=0.95))  # finds nothing
    truth, data = node_data(orc, 0.35)
    qs.append(dict(kind="MatchWith3DofInitial", sm=1, pose_in_submap_guess=guess_3dof(truth, 2),
                   data=dict(data, high_resolution_point_cloud=np.zeros((0, 3), np.float32)), min_score=0.2))  # empty
    qs.append(dict(qs[1]))  # a duplicate
    return qs


def with_matchers(qs, scene):
    return [dict(q, matcher=scene[q["sm"]].dm) for q in qs]


def test_mixed_batch_equals_single_calls_and_oracle(dl, ctx, orc, scene):
    qs = with_matchers(mixed_queries(orc, scene), scene)
    # MatchFullSubmap on the reference test's small scene (a whole-submap window over a 12-point cloud)
    g = orc.HybridGrid(0.05)
    hit, miss = orc.lookup_table_to_apply_odds(orc.odds(0.7)), orc.lookup_table_to_apply_odds(orc.odds(0.4))
    pose = np.array([0.3, -0.2, 0.1, np.cos(0.05), 0, 0, np.sin(0.05)], np.float32)
    g.insert_tables(pose[:3], orc.transform_points(pose, KAT_CLOUD), hit, miss, 5)
    dg = to_device_grid(dl, ctx, g)
    hist = np.zeros((1, 10), np.float32)
    om_k = orc.FastCorrelativeScanMatcher3D(g, g, hist, [0.1], KAT_OPTS)
    dm_k = dl.FastCorrelativeScanMatcher3D(ctx, dg, dg, hist, [0.1], KAT_OPTS)
    kat = dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=KAT_CLOUD, low_resolution_point_cloud=KAT_CLOUD,
               rotational_scan_matcher_histogram=np.zeros(10, np.float32))
    qs.append(dict(kind="MatchFullSubmap", matcher=dm_k, global_node_rotation=IDENT[3:], global_submap_rotation=IDENT[3:],
                   data=kat, min_score=0.1))
    results, statuses, stats = dl.fast_csm_match_batch(ctx, qs)
    assert statuses == [0] * len(qs)
    found = 0
    for q, r in zip(qs, results):
        same_result(r, single(q["matcher"], q))
        same_result(r, oracle_of(scene[q["sm"]].om if "sm" in q else om_k, q))
        found += r["found"]
    assert 0 < found < len(qs)
    assert stats["batched"] + stats["per_query"] + stats["without_search"] == len(qs)
    assert stats["without_search"] >= 1  # the empty cloud
    dm_k.close()
    dg.close()


def test_batch_argument_checks(dl, ctx, orc, scene):
    import ctypes as C
    L = dl.load_library()
    res = (dl.FastCsmResult * 1)()
    st = (C.c_int * 1)()
    assert L.dliom_fast_csm_match_batch(ctx.h, None, 1, res, st, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_fast_csm_match_batch(ctx.h, None, 0, None, None, None) == dl.OK
    q = (dl.FastCsmQuery * 1)()
    truth, data = node_data(orc, 0.25)
    q[0].kind = dl.FAST_CSM_MATCH_WITH_3DOF_INITIAL
    q[0].matcher = scene[0].dm.h
    q[0].pose[:] = list(truth)
    q[0].node_data = scene[0].dm._data(data)
    q[0].min_score = 0.2
    q[0].histogram_size = scene[0].dm.hist_size + 1  # not the matcher's
    assert L.dliom_fast_csm_match_batch(ctx.h, q, 1, res, st, None) == dl.ERR_INVALID_ARGUMENT
    q[0].histogram_size = scene[0].dm.hist_size
    q[0].kind = 7
    assert L.dliom_fast_csm_match_batch(ctx.h, q, 1, res, st, None) == dl.ERR_INVALID_ARGUMENT
    q[0].kind = dl.FAST_CSM_MATCH_WITH_3DOF_INITIAL
    assert L.dliom_fast_csm_match_batch(ctx.h, q, 1, res, st, None) == dl.OK
    assert L.dliom_csm3d_match_batch(ctx.h, None, 1, None, None, None, None, None) == dl.ERR_INVALID_ARGUMENT


def test_order_and_chunk_invariance(dl, ctx, orc, scene):
    qs = with_matchers(mixed_queries(orc, scene), scene)
    want, _, _ = dl.fast_csm_match_batch(ctx, qs)
    perm = np.random.RandomState(7).permutation(len(qs))
    got, _, _ = dl.fast_csm_match_batch(ctx, [qs[i] for i in perm])
    for j, i in enumerate(perm):
        same_result(got[j], want[i])
    big = [qs[i % len(qs)] for i in range(512)]
    got, statuses, stats = dl.fast_csm_match_batch(ctx, big)
    assert statuses == [0] * len(big)
    assert stats["chunks"] >= 2 and stats["frontier_chains"] == stats["chunks"]
    for i, r in enumerate(got):
        same_result(r, want[i % len(qs)])


def fast_found(dl, ctx, orc, scene, n):
    qs = with_matchers(mixed_queries(orc, scene), scene)
    results, _, _ = dl.fast_csm_match_batch(ctx, qs)
    return [(q, r) for q, r in zip(qs, results) if r["found"]][:n]


def test_csm_batch_equals_single_and_oracle(dl, ctx, orc, scene):
    from dliom import synth
    pairs = fast_found(dl, ctx, orc, scene, 8)
    assert len(pairs) >= 4
    for yaw_only in (False, True):
        copts = dict(DEFAULT_CSM, only_optimize_yaw=yaw_only)
        csm = dl.CeresScanMatcher3D(ctx, copts)
        problems, oracle_grids = [], []
        for q, r in pairs:
            sm = scene[q["sm"]]
            problems.append((r["pose"][:3], r["pose"], [(q["data"]["high_resolution_point_cloud"], sm.g_hi),
                                                        (q["data"]["low_resolution_point_cloud"], sm.g_lo)]))
            oracle_grids.append((sm.og_hi, sm.og_lo))
        if not yaw_only:  # one problem above the one-launch limit (4 096 points)
            pts, _ = synth.scan(synth.trajectory_pose(0.3), 32, 256)
            init = synth.perturb_pose(synth.trajectory_pose(0.3), 0.05, 0.5, seed=2)
            problems.append((init[:3], init, [(pts, scene[0].g_hi), (pts[::2], scene[0].g_lo)]))
            oracle_grids.append((scene[0].og_hi, scene[0].og_lo))
        poses, summaries, statuses, stats = csm.match_batch(problems)
        assert statuses == [0] * len(problems)
        assert stats["lm_launches"] == 1 and stats["batched"] == len(pairs)
        assert stats["per_query_one_launch"] == (0 if yaw_only else 1)
        for (tgt, init, cg), p, s, (oh, ol) in zip(problems, poses, summaries, oracle_grids):
            p1, s1 = csm.Match(tgt, init, cg)
            assert np.array_equal(p, p1) and s == s1
            ro = orc.csm3d_match(copts, tgt, init, [(cg[0][0], oh), (cg[1][0], ol)])
            assert np.linalg.norm(p[:3] - ro["pose"][:3]) <= 1e-6
            dt, dr = pose_distance(p, ro["pose"])
            assert dt <= 1e-6 and dr <= 1e-6
            assert s["num_iterations"] == ro["num_iterations"]


def test_compute_constraints_equals_oracle_chain(dl, ctx, orc, scene):
    """Every third node of submap A (scans 0-5) against submap B (scans 3-8): MatchWith3DofInitial, prune, refine."""
    from dliom import synth
    b = scene[1]
    copts = dict(DEFAULT_CSM)
    csm = dl.CeresScanMatcher3D(ctx, copts)
    qs = []
    for node in range(0, 6 * 3, 3):
        truth, data = node_data(orc, 0.1 * node / 3.0 + 0.02)
        guess = guess_3dof(truth, node) if node % 2 == 0 else synth.perturb_pose(truth, 2.5, 3.0, seed=node)
        qs.append(dict(kind="MatchWith3DofInitial", matcher=b.dm, pose_in_submap_guess=guess, data=data,
                       min_score=0.3 + 0.02 * (node % 4)))
    out, fast_stats, csm_stats = dl.compute_constraints(ctx, qs, csm)
    found = pruned = 0
    for q, c in zip(qs, out):
        ro = b.om.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"])
        assert (c is not None) == ro["found"]
        if c is None:
            pruned += 1
            continue
        found += 1
        same_result(c["match"], ro)
        rc = orc.csm3d_match(copts, ro["pose"][:3], ro["pose"], [(q["data"]["high_resolution_point_cloud"], b.og_hi),
                                                                (q["data"]["low_resolution_point_cloud"], b.og_lo)])
        assert np.linalg.norm(c["pose"][:3] - rc["pose"][:3]) <= 1e-6
        dt, dr = pose_distance(c["pose"], rc["pose"])
        assert dt <= 1e-6 and dr <= 1e-6
    assert found > 0 and pruned > 0


def test_batch_is_one_pass(dl, ctx, orc, scene):
    """64 eligible 3-DoF queries: one frontier chain, one LM launch, nothing on the per-query path, and fewer than a
    quarter of the host round trips the 64 single calls make."""
    # D-LIOM's constraint-builder options (basic_config_3d.lua:115-135 over pose_graph.lua) on submap A's grids
    dliom_opts = dict(branch_and_bound_depth=8, full_resolution_depth=3, min_rotational_score=0.6,
                      min_low_resolution_score=0.55, linear_xy_search_window=15.0, linear_z_search_window=8.0,
                      angular_search_window=np.deg2rad(45.0))
    sm = scene[0]
    from dliom import synth
    hists = [orc.compute_histogram(synth.scan(synth.trajectory_pose(0.1 * s), 16, 256)[0], 30) for s in range(6)]
    yaws = [yaw_of(synth.trajectory_pose(0.1 * s)) for s in range(6)]
    m = dl.FastCorrelativeScanMatcher3D(ctx, sm.g_hi, sm.g_lo, np.array(hists), yaws, dliom_opts)
    qs = []
    for k in range(64):
        truth, data = node_data(orc, 0.05 * (k % 8) + 0.2)
        qs.append(dict(kind="MatchWith3DofInitial", matcher=m, pose_in_submap_guess=guess_3dof(truth, k), data=data,
                       min_score=0.45))
    c2 = dl.Context(0)
    rb0, sy0 = c2.read_backs(), c2.synchronizations()
    serial = [single(m, q, ctx=c2) for q in qs]
    single_trips = (c2.read_backs() - rb0) + (c2.synchronizations() - sy0)
    c2.close()
    csm = dl.CeresScanMatcher3D(ctx, DEFAULT_CSM)
    out, fast_stats, csm_stats = dl.compute_constraints(ctx, qs, csm)
    for c, r in zip(out, serial):
        assert (c is not None) == r["found"]
        if c is not None:
            same_result(c["match"], r)
    assert fast_stats["frontier_chains"] == 1 and fast_stats["per_query"] == 0 and fast_stats["batched"] == 64
    assert csm_stats["lm_launches"] == 1 and csm_stats["per_query"] == 0
    batch_trips = fast_stats["synchronizations"] + fast_stats["read_backs"]
    assert batch_trips * 4 < single_trips, (batch_trips, single_trips, fast_stats)
    assert any(c is not None for c in out)
    m.close()


def test_cpp_adapter_compute_constraints(dl, tmp_path):
    exe = str(tmp_path / "constraint_batch_adapter")
    libdir = os.path.join(ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "constraint_batch_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
