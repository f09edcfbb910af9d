"""Fuzzes the device 2D probability grid against the CPU oracle: random resolutions (0.02 .. 1 m), origins, batch sizes
(0 .. 5000), point distributions (uniform, ring, snapped to half pixels, collinear, one pixel), random
insert_free_space, several batches per grid; limits, every cell, the cropped box and the error word are compared after
every batch (tests/probability_grid_common.py assert_equal).  No generator produces a case the oracle would abort on, so
none may be skipped.

    python tools/fuzz_probability_grid.py --seed 7 --cases 200
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import probability_grid_common as pc  # noqa: E402

f32 = np.float32


def make_points(rng, kind, n, origin, resolution, reach):
    if kind == "uniform":
        pts = origin + rng.uniform(-reach, reach, (n, 3))
    elif kind == "ring":
        a = rng.uniform(0, 2 * np.pi, n)
        d = reach * rng.uniform(0.8, 1.0, n)
        pts = origin + np.stack([d * np.cos(a), d * np.sin(a), rng.uniform(-1, 1, n)], axis=1)
    elif kind == "half_pixel":  # what reaches sub_y == denominator and sub_y == 0
        pts = np.round((origin + rng.uniform(-reach, reach, (n, 3))) / (resolution / 2)) * (resolution / 2)
    elif kind == "collinear":
        direction = rng.uniform(-1, 1, 3)
        pts = origin + np.outer(rng.uniform(-reach, reach, n), direction)
    else:  # one pixel
        pts = origin + rng.uniform(-reach, reach, 3) + rng.uniform(0, 0.3 * resolution, (n, 3))
    return pts.astype(f32)


def make_case(rng):
    resolution = float(rng.choice([0.02, 0.05, 0.1, 0.25, 0.5, 1.0, float(rng.uniform(0.02, 1.0))]))
    free = bool(rng.randint(2))
    hit, miss = float(rng.uniform(0.51, 0.9)), float(rng.uniform(0.1, 0.49))
    batches = []
    for _ in range(rng.randint(1, 5)):
        origin = rng.uniform(-20, 20, 3) * resolution * 4
        if rng.randint(4) == 0:
            origin = np.round(origin / (resolution / 2)) * (resolution / 2)
        n = int(rng.choice([0, 1, 2, rng.randint(3, 200), rng.randint(200, 5001)]))
        kind = str(rng.choice(["uniform", "ring", "half_pixel", "collinear", "one_pixel"]))
        reach = resolution * float(rng.choice([0.4, 3, 40, 400]))  # at most 800 cells from the origin
        batches.append((origin.astype(f32), make_points(rng, kind, n, origin, resolution, reach)))
    return resolution, hit, miss, free, batches


def run(dl, orc, ctx, seed, cases):
    rng = np.random.RandomState(seed)
    # `skipped` stays 0 by construction: there is no skip path, every generated case is inserted and compared
    report = dict(seed=seed, cases=0, skipped=0, inserts=0, points=0, growths=0, cells_visited=0)
    for _ in range(cases):
        resolution, hit, miss, free, batches = make_case(rng)
        grid = dl.ProbabilityGrid2D(ctx, resolution)
        ins = dl.Inserter2D(ctx, hit, miss, free)
        ogrid = pc.new_oracle_grid(orc, resolution)
        for origin, pts in batches:
            ins.insert(grid, origin, pts)
            ogrid.insert(origin, pts, hit, miss, free)
            pc.assert_equal(grid, ogrid)
            report["inserts"] += 1
            report["points"] += len(pts)
        s = grid.stats()
        report["growths"] += s["growths"]
        report["cells_visited"] += s["cells_visited"]
        report["cases"] += 1
        ins.close()
        grid.close()
    assert report["skipped"] == 0
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=100)
    a = ap.parse_args()
    import dliom as dl
    from oracle import oracle as orc
    ctx = dl.Context(0)
    print(json.dumps(run(dl, orc, ctx, a.seed, a.cases)))
    ctx.close()


if __name__ == "__main__":
    main()
