#!/usr/bin/env python3
"""Randomised differential test of the batched loop-closure constraints (dliom_fast_csm_match_batch and
dliom_csm3d_match_batch) against the single calls and the CPU oracle.  Each case builds 1 to 4 matchers on their own
submaps (cube or yard scene, random resolution, pyramid depth 1-7, thresholds, windows, histogram size) and sends one
batch of up to 40 Match / MatchFullSubmap / MatchWith3DofInitial queries over them in random order, with duplicates.
High-resolution clouds sometimes hold 1, 2047-2049 (kScoreChunk) or 8192/8193 (kFrontierMaxPoints) points, low-resolution
clouds 1 or 63-65 (pad64); a low-resolution cloud of 0 points must be refused by the batch and the single call alike.
The found matches are then refined by CeresScanMatcher3D.match_batch under a random option set with 1-3 clouds per
problem (device clouds and host arrays, grids of different resolutions)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = ("Match", "MatchFullSubmap", "MatchWith3DofInitial")
HI_SIZES = (1, 30, 150, 400, 2047, 2048, 2049, 8192, 8193)
LO_SIZES = (1, 63, 64, 65, 90)


def same_fast(a, b):
    if a["found"] != b["found"] or a["num_discrete_scans"] != b["num_discrete_scans"]:
        return False
    if not a["found"]:
        return True
    return (np.float32(a["score"]) == np.float32(b["score"]) and np.array_equal(a["pose"], b["pose"]) and
            np.float32(a["rotational_score"]) == np.float32(b["rotational_score"]) and
            np.float32(a["low_resolution_score"]) == np.float32(b["low_resolution_score"]))


def single_call(m, q):
    if q["kind"] == "Match":
        return m.Match(q["global_node_pose"], q["global_submap_pose"], q["data"], q["min_score"])
    if q["kind"] == "MatchFullSubmap":
        return m.MatchFullSubmap(q["global_node_rotation"], q["global_submap_rotation"], q["data"], q["min_score"])
    return m.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"])


def num_scans_bound(res, max_norm, angular_window):
    """GenerateDiscreteScans' scan count before the rotational filter."""
    r = max(float(max_norm), 3.0 * res)
    step = 0.99 * np.arccos(1.0 - res * res / (2.0 * r * r))
    return 2 * int(round(angular_window / step)) + 1


def lowest_count(linear_xy, linear_z, depth, scans):
    step = 1 << (depth - 1)
    return ((2 * linear_xy + step) // step) ** 2 * ((2 * linear_z + step) // step) * scans


def take(rng, pts, n):
    """n points of pts (with repeats once pts runs out), in a random order."""
    if n <= len(pts):
        return pts[rng.choice(len(pts), n, replace=False)]
    return pts[rng.choice(len(pts), n, replace=True)]


class Matcher:
    def __init__(self, dl, ctx, orc, synth, rng):
        from helpers import build_oracle_submap, to_device_grid
        self.res = float(rng.choice([0.1, 0.15, 0.2, 0.25, 0.3]))
        self.lo_res = float(rng.choice([0.4, 0.5, 0.6]))
        self.first = int(rng.randint(0, 6))
        scans = int(rng.randint(2, 5))
        self.og_hi = build_oracle_submap(orc, self.res, num_scans=scans, beams=8, azimuths=128, max_range=15.0,
                                         first_scan=self.first)
        self.og_lo = build_oracle_submap(orc, self.lo_res, num_scans=scans, beams=8, azimuths=128, first_scan=self.first)
        self.g_hi, self.g_lo = to_device_grid(dl, ctx, self.og_hi), to_device_grid(dl, ctx, self.og_lo)
        self.depth = int(rng.randint(1, 8))
        self.opts = dict(branch_and_bound_depth=self.depth, full_resolution_depth=int(rng.randint(1, self.depth + 1)),
                         min_rotational_score=float(rng.uniform(0.0, 0.8)),
                         min_low_resolution_score=float(rng.uniform(0.05, 0.5)),
                         linear_xy_search_window=float(rng.uniform(0.2, 3.0)),
                         linear_z_search_window=float(rng.uniform(0.1, 1.2)),
                         angular_search_window=float(np.deg2rad(rng.uniform(0.5, 30.0))))
        self.hsize = int(rng.choice([10, 30, 120]))
        self.span = (0.1 * self.first, 0.1 * (self.first + scans - 1))
        hists, yaws = [], []
        for s in range(self.first, self.first + scans):
            pts, _ = synth.scan(synth.trajectory_pose(0.1 * s), 8, 128)
            hists.append(orc.compute_histogram(pts, self.hsize))
            yaws.append(float(rng.uniform(-0.2, 0.2)))
        self.om = orc.FastCorrelativeScanMatcher3D(self.og_hi, self.og_lo, np.array(hists), yaws, self.opts)
        self.dm = dl.FastCorrelativeScanMatcher3D(ctx, self.g_hi, self.g_lo, np.array(hists), yaws, self.opts)
        self.lxy = int(round(self.opts["linear_xy_search_window"] / self.res))
        self.lz = int(round(self.opts["linear_z_search_window"] / self.res))
        self.width = 64 << self.g_hi.bits

    def cost(self, kind, max_norm, n_hi):
        """(lowest-resolution candidates, full-resolution lookups of an exhaustive search): what the oracle may spend on a
        query.  A whole-submap window is only bounded below; its queries are also gated on a measured cost."""
        if kind == "MatchFullSubmap":
            w = (self.width + 1) // 2 + int(np.floor(max_norm / self.res + 1.0))
            return lowest_count(w, w, self.depth, num_scans_bound(self.res, max_norm, np.pi)), 0
        scans = 1 if kind == "MatchWith3DofInitial" else num_scans_bound(self.res, max_norm, self.opts["angular_search_window"])
        full = (2 * self.lxy + 1) ** 2 * (2 * self.lz + 1) * scans
        return lowest_count(self.lxy, self.lz, self.depth, scans), full * max(n_hi, 1)

    def close(self):
        self.dm.close()
        self.g_hi.close()
        self.g_lo.close()


def node_query(rng, orc, synth, m, kind, big_scan, hi_n, lo_n):
    """One query on matcher m: a scan from inside the submap's span, its clouds cut to hi_n / lo_n points."""
    t = float(rng.uniform(m.span[0], m.span[1] + 0.1))
    truth = synth.trajectory_pose(t)
    pts, _ = synth.scan(truth, 8, 128)
    if kind == "MatchFullSubmap":  # the nearest returns only: a small whole-submap search
        near = pts[np.argsort(np.linalg.norm(pts, axis=1))[:max(hi_n, 1) * 3]]
        hi = take(rng, near, hi_n)
    else:
        hi = take(rng, big_scan(truth) if hi_n > len(pts) else pts, hi_n)
    lo = take(rng, pts[::3], lo_n)
    g = synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0, 0.05))
    data = dict(gravity_alignment=g, high_resolution_point_cloud=hi, low_resolution_point_cloud=lo,
                rotational_scan_matcher_histogram=orc.compute_histogram(pts, m.hsize))
    q = dict(kind=kind, matcher=m.dm, data=data, min_score=float(rng.uniform(0.05, 0.7)))
    if kind == "Match":
        q["global_node_pose"] = synth.perturb_pose(truth, float(rng.uniform(0, 1.5)), float(rng.uniform(0, 8.0)),
                                                   seed=int(rng.randint(1 << 30)))
        q["global_submap_pose"] = synth.perturb_pose(np.array([0, 0, 0, 1.0, 0, 0, 0]), 0.3, 3.0, seed=int(rng.randint(1 << 30)))
    elif kind == "MatchFullSubmap":
        q["global_node_rotation"] = synth.perturb_pose(truth, 0.0, 5.0, seed=int(rng.randint(1 << 30)))[3:]
        q["global_submap_rotation"] = synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0, 0.05))
    else:
        guess = np.array(truth, dtype=np.float64).copy()
        guess[:3] += rng.uniform(-0.5, 0.5, size=3) * np.array([1.0, 1.0, 0.3])
        q["pose_in_submap_guess"] = guess
    return q


def draw_queries(rng, orc, synth, matchers, big_scan):
    qs, owners = [], []
    for _ in range(int(rng.randint(1, 41))):
        if qs and rng.rand() < 0.15:  # a duplicate of an earlier query
            k = int(rng.randint(len(qs)))
            qs.append(dict(qs[k]))
            owners.append(owners[k])
            continue
        mi = int(rng.randint(len(matchers)))
        m = matchers[mi]
        kind = KINDS[int(rng.randint(3))]
        hi_n = int(rng.choice(HI_SIZES)) if rng.rand() < 0.5 else int(rng.randint(20, 300))
        lo_n = int(rng.choice(LO_SIZES)) if rng.rand() < 0.5 else int(rng.randint(2, 120))
        if kind == "MatchFullSubmap":
            hi_n = min(hi_n, int(rng.randint(1, 80)))
        for _attempt in range(3):  # keep the oracle cheap: shrink the cloud, then fall back to a 3-DoF query
            q = node_query(rng, orc, synth, m, kind, big_scan, hi_n, lo_n)
            hi = q["data"]["high_resolution_point_cloud"]
            low, lookups = m.cost(kind, np.max(np.linalg.norm(hi, axis=1)) if len(hi) else 0.0, len(hi))
            if kind == "MatchFullSubmap" and low <= 2e4:
                # the whole-submap window prunes or not depending on the scene: gate on what the single call scored
                lookups = single_call(m.dm, q)["num_scored_candidates"] * max(len(hi), 1)
            if low <= 5e4 and lookups <= 2e7:
                break
            hi_n = max(1, hi_n // 8)
            if _attempt == 1:
                kind = "MatchWith3DofInitial"
        else:
            continue
        qs.append(q)
        owners.append(mi)
    return qs, owners


def refine(dl, ctx, orc, rng, matchers, qs, owners, results, log):
    """The found matches through CeresScanMatcher3D.match_batch: each equals Match() bit for bit and the oracle within
    1e-6 m / 1e-6 rad with the same iteration count."""
    from helpers import pose_distance
    found = [i for i, r in enumerate(results) if r["found"]]
    if not found:
        return 0, True
    ncl = int(rng.randint(1, 4))
    copts = dict(occupied_space_weight=[float(rng.uniform(0.5, 8.0)) for _ in range(ncl)],
                 translation_weight=float(rng.uniform(0.5, 10.0)), rotation_weight=float(rng.choice([4e2, 1e2, 40.0])),
                 only_optimize_yaw=bool(rng.rand() < 0.3), use_nonmonotonic_steps=bool(rng.rand() < 0.3),
                 max_num_iterations=int(rng.choice([1, 2, 12])))
    csm = dl.CeresScanMatcher3D(ctx, copts)
    problems, oracle_pairs, host_pairs, own = [], [], [], []
    for i in found:
        m = matchers[owners[i]]
        d = qs[i]["data"]
        choices = [(d["high_resolution_point_cloud"], m.g_hi, m.og_hi), (d["low_resolution_point_cloud"], m.g_lo, m.og_lo)]
        other = matchers[int(rng.randint(len(matchers)))]
        choices.append((d["high_resolution_point_cloud"], other.g_lo, other.og_lo))
        picks = [choices[k] for k in rng.permutation(3)[:ncl]]
        pairs = []
        for pts, g, _ in picks:
            if rng.rand() < 0.4:
                c = dl.PointCloud(ctx, pts)
                own.append(c)
                pairs.append((c, g))
            else:
                pairs.append((pts, g))
        pose = results[i]["pose"]
        problems.append((pose[:3], pose, pairs))
        host_pairs.append([(pts, g) for pts, g, _ in picks])
        oracle_pairs.append([(pts, og) for pts, _, og in picks])
    poses, summaries, statuses, stats = csm.match_batch(problems)
    ok = statuses == [0] * len(problems) and stats["batched"] + stats["per_query"] == len(problems)
    if not ok:
        log("MISMATCH refinement statuses", statuses, stats, copts)
    for k, ((tgt, init, pairs), p, s) in enumerate(zip(problems, poses, summaries)):
        if not ok:
            break
        p1, s1 = csm.Match(tgt, init, pairs if all(isinstance(c, dl.PointCloud) for c, _ in pairs) else host_pairs[k])
        ro = orc.csm3d_match(copts, tgt, init, oracle_pairs[k])
        dt, dr = pose_distance(p, ro["pose"])
        if not (np.array_equal(p, p1) and s == s1):
            log("MISMATCH refinement vs single, problem", k, "query", found[k], copts, p, p1, s, s1)
            ok = False
        elif not (dt <= 1e-6 and dr <= 1e-6 and s["num_iterations"] == ro["num_iterations"]):
            log("MISMATCH refinement vs oracle, problem", k, "query", found[k], copts, p, ro["pose"], dt, dr,
                s["num_iterations"], ro["num_iterations"])
            ok = False
    for c in own:
        c.close()
    return len(problems), ok


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--seed", type=int, default=97000)
    ap.add_argument("--seconds", type=float, default=120.0)
    args = ap.parse_args(argv)
    import dliom as dl
    from dliom import synth
    from oracle import oracle as orc
    ctx = dl.Context(0)
    t0 = time.time()
    done = queries = refined = 0

    def log(*a):
        print(*a)

    try:
        for case in range(args.cases):
            if time.time() - t0 > args.seconds:
                break
            seed = args.seed + case
            rng = np.random.RandomState(seed)
            synth.set_scene("ground" if rng.rand() < 0.35 else "cube")
            matchers = [Matcher(dl, ctx, orc, synth, rng) for _ in range(int(rng.randint(1, 5)))]
            big = {}

            def big_scan(truth):
                key = tuple(np.round(truth, 9))
                if key not in big:
                    big[key] = synth.scan(truth, 32, 512)[0]
                return big[key]

            qs, owners = draw_queries(rng, orc, synth, matchers, big_scan)
            results, statuses, stats = dl.fast_csm_match_batch(ctx, qs)
            fail = None
            if stats["batched"] + stats["per_query"] + stats["without_search"] != len(qs) or statuses != [0] * len(qs):
                fail = ("stats / statuses", statuses, stats)
            for i, (q, r) in enumerate(zip(qs, results)):
                if fail:
                    break
                m = matchers[owners[i]]
                rs, ro = single_call(m.dm, q), single_call(m.om, q)
                if not (same_fast(r, rs) and same_fast(r, ro)):
                    fail = ("query", i, "of", len(qs), q["kind"], "matcher", owners[i], m.opts, "min_score", q["min_score"],
                            "hi", len(q["data"]["high_resolution_point_cloud"]), "lo",
                            len(q["data"]["low_resolution_point_cloud"]), "batch", r, "single", rs, "oracle", ro)
            if fail is None and rng.rand() < 0.15 and qs:  # a 0-point low-resolution cloud: refused by both
                k = int(rng.randint(len(qs)))
                bad = dict(qs[k], data=dict(qs[k]["data"], low_resolution_point_cloud=np.zeros((0, 3), np.float32)))
                codes = []
                for call in (lambda: dl.fast_csm_match_batch(ctx, qs[:k] + [bad]), lambda: single_call(bad["matcher"], bad)):
                    try:
                        call()
                        codes.append(0)
                    except dl.DliomError as e:
                        codes.append(e.status)
                if codes != [dl.ERR_INVALID_ARGUMENT] * 2:
                    fail = ("empty low-resolution cloud", codes)
            if fail is None:
                n, ok = refine(dl, ctx, orc, rng, matchers, qs, owners, results, log)
                refined += n
                if not ok:
                    fail = ("refinement",)
            for m in matchers:
                m.close()
            synth.set_scene("cube")
            if fail is not None:
                print("MISMATCH seed", seed, "case", case, *fail)
                return 1
            done += 1
            queries += len(qs)
    finally:
        synth.set_scene("cube")
        ctx.close()
    print("constraint batch fuzz ok: %d cases, %d queries, %d refined problems in %.1f s" %
          (done, queries, refined, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
