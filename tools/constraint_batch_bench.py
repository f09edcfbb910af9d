#!/usr/bin/env python3
"""Loop-closure constraints (ConstraintBuilder3D::ComputeConstraint, constraint_builder_3d.cc:202-334) per second:
serial single calls on one context, 8 threads with a context each (the C++ adapter's Context::ForThisThread pattern)
and the batch (dliom.compute_constraints).  D-LIOM's constraint-builder options (basic_config_3d.lua:115-135 over
pose_graph.lua's constraint_builder): 0.2 m / 0.45 m grids, depth 8 / full-resolution depth 3, 15 m x 8 m x 45 deg,
min_score 0.45; ceres_scan_matcher_3d weights 5 / 30, translation 10, rotation 1, 10 iterations.  Two overlapping
synthetic submaps; every third node of A as a 3-DoF query against B (K queries, cycling).  Every batched result is
checked against the serial one.  One JSON line."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FAST = dict(branch_and_bound_depth=8, full_resolution_depth=3, min_rotational_score=0.6, min_low_resolution_score=0.55,
            linear_xy_search_window=15.0, linear_z_search_window=8.0, angular_search_window=np.deg2rad(45.0))
CERES = dict(occupied_space_weight=[5.0, 30.0], translation_weight=10.0, rotation_weight=1.0, only_optimize_yaw=False,
             use_nonmonotonic_steps=False, max_num_iterations=10)
MIN_SCORE = 0.45


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,67,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    import dliom as dl
    from dliom import synth
    from helpers import build_oracle_submap, to_device_grid
    from oracle import oracle as orc

    ctx = dl.Context(0)
    # submap B (scans 10-19) is matched by nodes of submap A (scans 0-19: A and B overlap in 10-19)
    og_hi = build_oracle_submap(orc, 0.2, num_scans=10, beams=32, azimuths=512, max_range=60.0, first_scan=10)
    og_lo = build_oracle_submap(orc, 0.45, num_scans=10, beams=32, azimuths=512, first_scan=10)
    g_hi, g_lo = to_device_grid(dl, ctx, og_hi), to_device_grid(dl, ctx, og_lo)
    hists, yaws = [], []
    for s in range(10, 20):
        pose = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(pose, 32, 512)
        hists.append(orc.compute_histogram(pts, 120))
        yaws.append(float(np.arctan2(2 * (pose[3] * pose[6] + pose[4] * pose[5]), 1 - 2 * (pose[5] ** 2 + pose[6] ** 2))))
    matcher = dl.FastCorrelativeScanMatcher3D(ctx, g_hi, g_lo, np.array(hists), yaws, FAST)
    base = []
    for node in range(0, 201, 3):  # num_range_data = 100 per submap: every third node of A's ~200 insertions
        t = 0.01 * node
        truth = synth.trajectory_pose(t)
        pts, _ = synth.scan(truth, 32, 512)
        data = dict(gravity_alignment=[1, 0, 0, 0], high_resolution_point_cloud=orc.adaptive_voxel_filter(2.0, 150, 15.0, pts),
                    low_resolution_point_cloud=orc.adaptive_voxel_filter(4.0, 200, 60.0, pts),
                    rotational_scan_matcher_histogram=orc.compute_histogram(pts, 120))
        guess = synth.perturb_pose(truth, 0.5, 2.0, seed=node)
        base.append(dict(kind="MatchWith3DofInitial", matcher=matcher, pose_in_submap_guess=guess, data=data,
                         min_score=MIN_SCORE))

    csm = dl.CeresScanMatcher3D(ctx, CERES)

    def one(q, c, cs):
        r = matcher.MatchWith3DofInitial(q["pose_in_submap_guess"], q["data"], q["min_score"], ctx=c)
        if not r["found"]:
            return None
        p, _ = cs.Match(r["pose"][:3], r["pose"], [(q["data"]["high_resolution_point_cloud"], g_hi),
                                                   (q["data"]["low_resolution_point_cloud"], g_lo)])
        return r, p

    pool = [dl.Context(0) for _ in range(args.threads)]
    pool_csm = [dl.CeresScanMatcher3D(c, CERES) for c in pool]
    out = {"workload": "ComputeConstraint x K (MatchWith3DofInitial + prune + CeresScanMatcher3D on both grids), "
                       "0.2 m submap of 10 scans, 15 m x 8 m x 45 deg, depth 8", "threads": args.threads, "sizes": {}}
    for K in [int(v) for v in args.sizes.split(",")]:
        qs = [base[i % len(base)] for i in range(K)]
        serial_t, pool_t, batch_t = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            serial = [one(q, ctx, csm) for q in qs]
            serial_t.append(time.perf_counter() - t0)
            got = [None] * K

            def worker(w):
                for i in range(w, K, args.threads):
                    got[i] = one(qs[i], pool[w], pool_csm[w])

            th = [threading.Thread(target=worker, args=(w,)) for w in range(args.threads)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            pool_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            batch, fast_stats, csm_stats = dl.compute_constraints(ctx, qs, csm)
            batch_t.append(time.perf_counter() - t0)
        same = True
        for s, b in zip(serial, batch):
            if (s is None) != (b is None):
                same = False
            elif s is not None:
                same &= bool(np.array_equal(s[0]["pose"], b["match"]["pose"]) and np.float32(s[0]["score"]) == b["match"]["score"]
                             and np.array_equal(s[1], b["pose"]))
        out["sizes"][str(K)] = {
            "constraints_per_s": {"serial": K / float(np.median(serial_t)), "pool_%d_contexts" % args.threads: K / float(np.median(pool_t)),
                                  "batch": K / float(np.median(batch_t))},
            "ms": {"serial": 1e3 * float(np.median(serial_t)), "pool": 1e3 * float(np.median(pool_t)),
                   "batch": 1e3 * float(np.median(batch_t))},
            "found": int(sum(b is not None for b in batch)), "batch_equals_serial": same,
            "fast_stats": fast_stats, "ceres_stats": csm_stats}
    print(json.dumps(out))
    for c in pool:
        c.close()
    ctx.close()


if __name__ == "__main__":
    main()
