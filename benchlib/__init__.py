"""bench.py's pieces outside the timed region (the timed loop is bench.py and nothing else).

  benchlib/__init__.py  constants, the scene (submap + scans), insertion targets
  benchlib/config5.py   BASELINE config 5: the --full line's `config5` at N = 1, the sharded line at N > 1
  benchlib/roofline.py  the `roofline` object: live rocprofv3 --pmc child runs of the same invocation
  benchlib/wref.py      the W-ref lines (tools/wref_full.py)
  benchlib/cpu_legs.py  the ONLY importer of oracle/: the post-timing parity check and the cpu_baseline leg
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "d-liom_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec); 6.29 TB/s measured copy
# MI355X_MICROARCH.md: 256 CUs x 4 SIMD-32, v_fma_f32 (wave64) = 2 cycles, 2.4 GHz
VALU_PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9

RTCSM_OPTS = dict(linear_search_window=0.15, angular_search_window=float(np.deg2rad(1.0)),
                  translation_delta_cost_weight=1e-1, rotation_delta_cost_weight=1e-1)
CSM_OPTS = dict(occupied_space_weight=[1.0, 6.0], translation_weight=5.0, rotation_weight=4e2,
                only_optimize_yaw=False, use_nonmonotonic_steps=False, max_num_iterations=12)
HIT_P, MISS_P, FREE = 0.55, 0.49, 2
HIGH_RES_MAX_RANGE = 20.0


SECOND_SUBMAP = []  # --config 5: the (hi, lo) grids of the second active submap, inserted into beside the matched one


def insertion_targets(g_hi, g_lo, pf):
    t = [(g_hi, [pf], HIGH_RES_MAX_RANGE), (g_lo, [pf], 0.0)]
    if SECOND_SUBMAP:
        t += [(SECOND_SUBMAP[0], [pf], HIGH_RES_MAX_RANGE), (SECOND_SUBMAP[1], [pf], 0.0)]
    return t


def build_scene(args, dl, synth, ctx):
    """Submap (map_scans scans inserted at ground truth) and the scans to match; the same on every rank."""
    ins = dl.RangeDataInserter3D(HIT_P, MISS_P, FREE, ctx=ctx)
    g_hi = dl.HybridGrid(ctx, args.high_resolution)
    g_lo = dl.HybridGrid(ctx, args.low_resolution)
    second = []
    if args.config == 5:
        # BASELINE config 5, "multi-submap insertion": TWO active submaps (submap_3d.cc:303-314) -- the newer one holds the
        # later half of the map scans -- and beams of +-35 degrees, so that returns reach the cube's corners (26 m) and the
        # search window is the one BASELINE.md section 3 states: C = 343 x 19^3 = 2 352 637
        synth.ELEVATION["cube"] = (-35.0, 35.0)
        second = [dl.HybridGrid(ctx, args.high_resolution), dl.HybridGrid(ctx, args.low_resolution)]
    SECOND_SUBMAP[:] = second
    centers = synth.bubbles()
    for s in range(args.map_scans):
        pose = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(pose, args.beams, args.azimuths, centers=centers)
        cloud = dl.PointCloud(ctx, pts)
        pf = pose.astype(np.float32)
        ins.InsertCloud(g_hi, cloud, poses=[pf], max_range=HIGH_RES_MAX_RANGE)
        ins.InsertCloud(g_lo, cloud, poses=[pf])
        if second and s >= args.map_scans // 2:
            ins.InsertCloud(second[0], cloud, poses=[pf], max_range=HIGH_RES_MAX_RANGE)
            ins.InsertCloud(second[1], cloud, poses=[pf])
        cloud.close()
    scans = []
    for k in range(args.distinct_scans):
        truth = synth.trajectory_pose(0.1 * (args.map_scans + k))
        pts, _ = synth.scan(truth, args.beams, args.azimuths, centers=centers)
        init = synth.perturb_pose(truth, 0.1, 0.5, seed=13 + k)
        scans.append(dict(truth=truth, pts=pts, init=init, cloud=dl.PointCloud(ctx, pts)))
    return ins, g_hi, g_lo, scans

