#!/usr/bin/env python3
"""Randomised differential test of the device outlier remover (dliom_outlier_remover_*) against the CPU model
(tests/cpp/outlier_model.cc).  Each case draws a voxel size in [0.02, 0.5], 2 to 5 batches with origins up to a few
hundred voxels apart and returns on shells around them (so that voxels collect several hits and other batches' rays pass
through them), plus a few rays as long as the grid's extent allows (8000 voxels), and compares the whole table, kept_index
and the kept points, all exactly.  The device counts pass 2 in a shuffled batch order: no count depends on it.
tests/test_gpu_outlier.py runs seeds 1-6; `--soak SECONDS` keeps drawing cases (one process, one GPU)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import outlier_common as oc  # noqa: E402

f32 = np.float32


def make_case(seed):
    rng = np.random.RandomState(seed)
    voxel_size = float(np.round(rng.uniform(0.02, 0.5), rng.randint(2, 7)))
    centre = rng.uniform(-300.0, 300.0, 3) * voxel_size
    shells = rng.uniform(5.0, 150.0, size=rng.randint(1, 4)) * voxel_size
    batches = []
    for _ in range(rng.randint(2, 6)):
        origin = (centre + rng.uniform(-40.0, 40.0, 3) * voxel_size).astype(f32)
        n = int(rng.choice([1, 63, 64, 65, 700, 3000]))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        # returns on shells around the common centre, seen from this origin
        target = centre + d * rng.choice(shells, n)[:, None] * rng.uniform(0.98, 1.02, (n, 1))
        pts = target.astype(f32)
        far = rng.randint(0, 4)  # rays up to the extent: |coordinate| <= 8000 voxels
        if far:
            long_rays = rng.uniform(-8000.0, 8000.0, (far, 3)) * voxel_size
            pts = np.concatenate([pts, long_rays.astype(f32)])
        if rng.rand() < 0.3:
            pts = np.concatenate([pts, np.tile(origin, (2, 1))])  # length 0
        batches.append((origin, pts[rng.permutation(len(pts))]))
    return voxel_size, batches


def run_case(dl, ctx, model, seed, directory):
    voxel_size, batches = make_case(seed)
    results, table = oc.run_model(model, voxel_size, oc.three_pass_ops(batches), directory)
    assert all((r if isinstance(r, int) else r[0]) == 0 for r in results), (seed, results)
    r = dl.OutlierRemover(ctx, voxel_size)
    clouds = [dl.PointCloud(ctx, p) for _, p in batches]
    for c in clouds:
        r.mark_hits(c)
    for i in np.random.RandomState(seed + 1000).permutation(len(batches)):
        r.count_rays(batches[i][0], clouds[i])
    xyz, hits, rays = r.voxels()
    assert np.array_equal(xyz, table[0]) and np.array_equal(hits, table[1]) and np.array_equal(rays, table[2]), seed
    removed = 0
    for (_, pts), c, (_, want) in zip(batches, clouds, results[2 * len(batches):]):
        kept, index = r.filter(c)
        assert np.array_equal(index, want) and kept.download().tobytes() == pts[want].tobytes(), seed
        removed += len(pts) - len(want)
        kept.close()
        c.close()
    stats = r.stats()
    r.close()
    return dict(seed=seed, voxel_size=voxel_size, batches=len(batches), points=sum(len(p) for _, p in batches),
                removed=removed, voxels=len(hits), voxels_with_rays=int((rays > 0).sum()), samples=stats["samples_walked"])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seeds", type=int, nargs="*", default=list(range(1, 21)))
    ap.add_argument("--soak", type=float, default=0.0, help="seconds to keep drawing cases after --seeds")
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    with tempfile.TemporaryDirectory() as d:
        model = oc.build_model(d)
        t0, seed, done = time.time(), 0, 0
        for seed in args.seeds:
            print(run_case(dl, ctx, model, seed, d), flush=True)
            done += 1
        while time.time() - t0 < args.soak:
            seed += 1
            print(run_case(dl, ctx, model, seed, d), flush=True)
            done += 1
    ctx.close()
    print("fuzz_outlier: %d cases equal" % done)


if __name__ == "__main__":
    main()
