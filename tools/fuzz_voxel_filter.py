#!/usr/bin/env python3
"""Randomised differential test of the device voxel filters (dliom_cloud_voxel_filter, _adaptive_voxel_filter, _pair)
against the CPU oracle.  Each seed draws a cloud of 1 to 300 000 points -- the size weighted towards the kernels' shapes
(256 per flag / compact workgroup, 1024 per insert workgroup, 65 536 = 256 compact workgroups, the powers of two at which
the hash table's capacity steps), the points uniform, clustered around a few centres, drawn with repetition from a few
points, or snapped to the voxel lattice and its half-way planes, now and then with one point beyond the packed table
words' 4095 edges -- an edge length, and two AdaptiveVoxelFilter option triples whose min_num_points is either random or
exactly a survivor count (or one more) at a length the search visits.  The plain filter, both adaptive filters alone and
the pair are compared with the oracle bit for bit.  A failing seed is printed.
tests/test_gpu_voxel_filter.py runs seeds 1-40 with the size capped; `--soak SECONDS` keeps drawing cases."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import voxel_filter_common as vc  # noqa: E402

f32 = np.float32
BOUNDARIES = [1, 64, 256, 1024, 2048, 4096, 16384, 32768, 65536, 65792, 131072, 262144]


def draw_n(rng, max_n):
    if rng.rand() < 0.6:
        n = int(rng.choice([b for b in BOUNDARIES if b <= max_n] or [1])) + int(rng.randint(-1, 3))
    else:
        n = int(np.exp(rng.uniform(0.0, np.log(max_n))))
    return int(min(max(n, 1), max_n))


def draw_cloud(rng, n, size):
    extent = float(rng.choice([2.0, 20.0, 80.0]))
    kind = rng.randint(0, 4)
    if kind == 0:  # uniform
        pts = rng.uniform(-extent, extent, size=(n, 3))
    elif kind == 1:  # a few tight clusters: many points per voxel, the same voxels in every workgroup
        centres = rng.uniform(-extent, extent, size=(rng.randint(1, 6), 3))
        pts = centres[rng.randint(0, len(centres), n)] + rng.normal(0.0, size * rng.choice([0.1, 0.5, 3.0]), size=(n, 3))
    elif kind == 2:  # bit-identical repetitions of a few points
        source = rng.uniform(-extent, extent, size=(rng.randint(1, 200), 3))
        pts = source[rng.randint(0, len(source), n)]
    else:  # on the lattice and on the half-way planes of the rounding
        pts = np.round(rng.uniform(-extent, extent, size=(n, 3)) / size * 2.0) / 2.0 * f32(size)
    pts = pts.astype(f32)
    if rng.rand() < 0.3:
        pts = pts[np.argsort(pts[:, rng.randint(0, 3)], kind="stable")]  # a voxel's points next to each other
    if rng.rand() < 0.15:  # beyond the 13 bits per axis of the packed words, inside the keys' 21
        pts[rng.randint(0, n), rng.randint(0, 3)] = f32(rng.choice([-1.0, 1.0]) * size * rng.uniform(4095.0, 9000.0))
    return np.ascontiguousarray(pts), extent


def draw_options(rng, orc, pts, extent):
    max_length = float(f32(np.round(10.0 ** rng.uniform(-1.0, 0.7), rng.randint(1, 4))))
    max_range = float(rng.choice([0.5 * extent, extent, 1.8 * extent, 4.0 * extent]))  # (<= 320 m: inside the 21-bit keys at max_length / 128)
    if rng.rand() < 0.5:
        t = rng.randint(1, len(pts) + 3)
    else:  # a tie of the search's `>=`, or one above it
        length = f32(f32(max_length) / f32(2 ** rng.randint(0, 8)) * f32(1.0 + rng.randint(0, 17) / 16.0))
        cropped = vc.crop(pts, max_range)
        t = (len(orc.voxel_filter(float(length), cropped)) if len(cropped) else 0) + rng.randint(0, 2)
    return (max_length, float(max(t, 1)), max_range)


def make_case(seed, orc, max_n=300000):
    rng = np.random.RandomState(seed)
    n = draw_n(rng, max_n)
    size = float(f32(np.round(10.0 ** rng.uniform(-1.7, 0.5), rng.randint(2, 5))))
    pts, extent = draw_cloud(rng, n, size)
    return pts, size, draw_options(rng, orc, pts, extent), draw_options(rng, orc, pts, extent)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def run_case(dl, ctx, orc, seed, max_n=300000):
    pts, size, first, second = make_case(seed, orc, max_n)
    cloud = dl.PointCloud(ctx, pts)
    want = pts[orc.voxel_filter(size, pts)]
    out = cloud.voxel_filter(size)
    got = out.download()
    out.close()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (seed, "plain", size)
    wants = [orc.adaptive_voxel_filter(o[0], o[1], o[2], pts) for o in (first, second)]
    a, b = cloud.adaptive_voxel_filter_pair(first, second)
    single = cloud.adaptive_voxel_filter(*first)
    for name, o, c, w in (("pair[0]", first, a, wants[0]), ("pair[1]", second, b, wants[1]), ("single", first, single, wants[0])):
        got = c.download()
        c.close()
        assert got.shape == w.shape and np.array_equal(bits(got), bits(w)), (seed, name, o)
    cloud.close()
    return dict(seed=seed, n=len(pts), size=size, kept=len(want), first=first, second=second,
                kept_first=len(wants[0]), kept_second=len(wants[1]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seeds", type=int, nargs="*", default=list(range(1, 41)))
    ap.add_argument("--max-n", type=int, default=300000)
    ap.add_argument("--soak", type=float, default=0.0, help="seconds to keep drawing cases after --seeds")
    ap.add_argument("--quiet", action="store_true", help="print only failures and the summary")
    args = ap.parse_args(argv)
    import dliom as dl
    from oracle import oracle as orc
    orc.lib()
    ctx = dl.Context(0)
    t0, seed, done = time.time(), 0, 0

    def one(seed):
        try:
            line = run_case(dl, ctx, orc, seed, args.max_n)
        except (AssertionError, dl.DliomError) as e:
            print("fuzz_voxel_filter: FAILED at seed %d (--seeds %d --max-n %d): %r" % (seed, seed, args.max_n, e), flush=True)
            return False
        if not args.quiet:
            print(line, flush=True)
        return True

    try:
        for seed in args.seeds:
            if not one(seed):
                return 1
            done += 1
        while time.time() - t0 < args.soak:
            seed += 1
            if not one(seed):
                return 1
            done += 1
    finally:
        ctx.close()
    print("voxel filter fuzz ok: %d cases equal" % done)
    return 0


if __name__ == "__main__":
    sys.exit(main())
