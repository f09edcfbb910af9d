#!/usr/bin/env python3
"""Painting submap slices into one map (dliom_submap_slices_paint / _occupancy: io::PaintSubmapSlices and
CreateOccupancyGridMsg) on the device against the CPU model of the statement (tests/submap_painter_common.py, numpy) and,
where the machine has libcairo, against cairo's own paint of the reference's call sequence on one thread.  The scene:
--slices slices of about --texels x --texels texels at 0.10 m on a 0.05 m map, laid out on a square lattice with overlap
and random yaw; then every slice gets a new pose (set_pose, no texture moves) and the map is painted again.  Prints the
map's size, the (tile, slice) pairs, the device ms per paint and per occupancy grid (pixels downloaded; median of --reps),
the model's and cairo's seconds, and checks the device against the model bit for bit.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(sp, n, texels, seed):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    pitch = 0.10 * texels * 0.5  # neighbours overlap by half
    slices = []
    for k in range(n):
        h, w = texels + int(rng.integers(-20, 21)), texels + int(rng.integers(-20, 21))
        pose = sp.yaw_pose(pitch * (k % side) + rng.uniform(-1, 1), pitch * (k // side) + rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi))
        slices.append(sp.make_slice(sp.random_cells(rng, h, w), 0.10, pose, sp.random_pose(rng, 2.0, 0.02)))
    return slices


def new_poses(sp, slices, seed):
    rng = np.random.default_rng(seed)
    for s in slices:
        s["pose"] = s["pose"].copy()
        s["pose"][:2] += rng.uniform(-0.3, 0.3, 2)
        s["pose"][3:] = sp.yaw_pose(0, 0, 2 * np.arctan2(s["pose"][6], s["pose"][3]) + rng.uniform(-0.02, 0.02))[3:]


def median_ms(call, reps):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--texels", type=int, default=600)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cairo", action="store_true")
    ap.add_argument("--skip-model", action="store_true", help="device times only, nothing checked (for a run under a profiler)")
    args = ap.parse_args()
    import dliom as dl
    import submap_painter_common as sp
    ctx = dl.Context(0)
    slices = scene(sp, args.slices, args.texels, 1)
    t = time.perf_counter()
    handles = [dl.SubmapSlice(ctx, s["cells"], s["resolution"], s["slice_pose"], s["pose"]) for s in slices]
    out = dict(slices=args.slices, texels=int(sum(s["cells"].shape[0] * s["cells"].shape[1] for s in slices)),
               resolution=args.resolution, upload_ms=1e3 * (time.perf_counter() - t))
    cairo = None if args.skip_cairo else sp.load_cairo()
    for phase in ("first", "after_set_pose"):
        if phase == "after_set_pose":
            new_poses(sp, slices, 2)
            t = time.perf_counter()
            for s, h in zip(slices, handles):
                h.set_pose(s["pose"])
            out["set_pose_ms"] = 1e3 * (time.perf_counter() - t)
        pixels, origin = dl.paint_submap_slices(ctx, handles, args.resolution)  # warm: scratch reserved
        stats = dl.submap_painter_stats(ctx)
        r = dict(width=int(pixels.shape[1]), height=int(pixels.shape[0]), launches=stats["launches"],
                 tile_slice_pairs=stats["tile_slice_pairs"])
        r["device_paint_ms"] = median_ms(lambda: dl.paint_submap_slices(ctx, handles, args.resolution), args.reps)
        r["device_occupancy_ms"] = median_ms(lambda: dl.submap_slices_occupancy(ctx, handles, args.resolution), args.reps)
        if not args.skip_model:
            t = time.perf_counter()
            status, want, want_origin, _, _ = sp.paint(slices, args.resolution, windowed=True)
            r["model_s"] = time.perf_counter() - t
            r["equal_model"] = bool(status == sp.OK and np.array_equal(pixels, want) and origin.tobytes() == want_origin.tobytes())
            data, origin_xy = dl.submap_slices_occupancy(ctx, handles, args.resolution)
            want_data, want_xy = sp.occupancy(want, want_origin, args.resolution)
            r["equal_model"] = r["equal_model"] and bool(np.array_equal(data, want_data) and origin_xy.tobytes() == want_xy.tobytes())
        if cairo is not None:
            t = time.perf_counter()
            cp, _ = sp.cairo_paint(cairo, slices, args.resolution)
            r["cairo_s"] = time.perf_counter() - t  # textures wrapped, bounding box, paint: what PaintSubmapSlices costs
            r["cairo_difference"], r["cairo_equal_share"] = sp.channel_differences(pixels, cp)
        out[phase] = r
    out["texels_uploaded"] = dl.submap_painter_stats(ctx)["texels_uploaded"]
    out["cairo"] = cairo.cairo_version_string().decode() if cairo is not None else None
    print(json.dumps(out))
    ok = args.skip_model or all(out[p]["equal_model"] for p in ("first", "after_set_pose"))
    for h in handles:
        h.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
