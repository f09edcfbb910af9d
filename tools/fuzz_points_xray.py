"""Randomised parity of the device X-ray aggregator (dliom_points_xray_*) against tests/cpp/points_xray_model.cc: random
voxel size, rigid transform, number of floors, batch sizes and colour modes, clustered points so that columns hold many
points and voxels, and now and then a batch the reference would abort on.  Everything is compared exactly
(tests/points_xray_common.py assert_equal).

    python tools/fuzz_points_xray.py [--seeds 1-50]

The GPU suite runs run_case() for a fixed list of seeds (tests/test_gpu_points_xray.py)."""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import points_xray_common as xc  # noqa: E402

f32 = np.float32


def make_case(seed):
    rng = np.random.RandomState(1000 + seed)
    voxel_size = float(rng.choice([0.03, 0.05, 0.07, 0.1, 0.15, 0.31]))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    transform = tuple(float(v) for v in np.r_[rng.uniform(-2, 2, 3), q].astype(f32))
    floors = int(rng.choice([1, 1, 2, 3]))
    centres = rng.uniform(-6, 6, (int(rng.randint(3, 40)), 3))
    ops = []
    for _ in range(int(rng.randint(2, 9))):
        n = int(rng.choice([0, 1, 7, 300, 5000, 40000, 70000]))
        spread = float(rng.choice([0.01, 0.2, 1.5]))
        pts = (centres[rng.randint(0, len(centres), n)] + rng.normal(size=(n, 3)) * spread).astype(f32)
        if rng.rand() < 0.3 and n > 0:  # a tall thin pile: many points and voxels in few columns
            pts[:, 1:] = (centres[0, 1:] + rng.normal(size=(n, 2)) * 0.03).astype(f32)
        mode = rng.randint(0, 3)
        colors = None if mode == 0 else (rng.uniform(0, 1, 3) if mode == 1 else rng.uniform(-0.2, 1.2, (n, 3)) *
                                         rng.choice([1.0, 1e-3, 1e3], (n, 1)))
        if mode == 2 and n == 0:
            colors = None
        if rng.rand() < 0.12 and n > 0:  # what the reference aborts on, somewhere in the batch
            # (20 000 cells along one axis leave the extent on some axis under every rotation: 20 000 / sqrt(3) > 8191)
            pts[rng.randint(0, n)] = np.array([1.0, rng.choice([np.nan, np.inf, 20000.0 * voxel_size]), 1.0])
        ops.append(xc.insert(pts, colors, aggregation=int(rng.randint(0, floors))))
    return voxel_size, transform, floors, ops


def run_case(dl, ctx, model, seed, directory):
    voxel_size, transform, floors, ops = make_case(seed)
    result, stats, _ = xc.compare(dl, ctx, model, voxel_size, transform, ops, directory, floors=floors, need_honest=False)
    return result, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="1-20")
    args = ap.parse_args()
    lo, _, hi = args.seeds.partition("-")
    import dliom
    ctx = dliom.Context(0)
    with tempfile.TemporaryDirectory() as d:
        model = xc.build_model(d)
        for seed in range(int(lo), int(hi or lo) + 1):
            result, stats = run_case(dliom, ctx, model, seed, d)
            print("seed %d: statuses %s columns %s longest %s" % (seed, result.statuses, [s["columns"] for s in stats],
                                                                  [s["longest_segment"] for s in stats]))
    ctx.close()


if __name__ == "__main__":
    main()
