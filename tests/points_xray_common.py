"""Shared by tests/test_points_xray_host.py, tests/test_gpu_points_xray.py, tools/fuzz_points_xray.py and
tools/points_xray_bench.py: builds and runs the CPU model (tests/cpp/points_xray_model.cc), makes the scenes, runs the
same operations on the device, and states when a comparison compares something (honest())."""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_common as oc  # noqa: E402

ROOT = oc.ROOT
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "points_xray_model.cc")
f32 = np.float32
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
# YZ_TRANSFORM, XY_TRANSFORM and XZ_TRANSFORM of the stock asset-writer configurations (transform.lua: roll, pitch, yaw =
# (0, 0, pi), (0, -pi/2, 0), (0, 0, -pi/2)) as [tx ty tz qw qx qy qz]: the quaternion of one rotation by `a` about an axis
# is (cos(a/2), axis * sin(a/2)) in double, rounded to float by Rigid3d::cast<float>().  cos(pi/2) is 6.123...e-17 in
# double, not 0.
TRANSFORMS = {"yz": (0.0, 0.0, 0.0, 6.123233995736766e-17, 0.0, 0.0, 1.0),
              "xy": (0.0, 0.0, 0.0, 0.7071067811865476, 0.0, -0.7071067811865475, 0.0),
              "xz": (0.0, 0.0, 0.0, 0.7071067811865476, 0.0, 0.0, -0.7071067811865475)}
WHITE = 0xFFFFFFFF


def build_model(directory):
    exe = os.path.join(str(directory), "points_xray_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def insert(points, colors=None, aggregation=0):
    """colors: None, one (r, g, b), or float32 (n, 3)."""
    pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    col = np.zeros((0, 3), dtype=f32) if colors is None else np.ascontiguousarray(colors, dtype=f32).reshape(-1, 3)
    assert len(col) in (0, 1, len(pts))
    return ("insert", aggregation, pts, col)


def pixels(occupied, max_occupied, means):
    return ("pixels", np.asarray(occupied, dtype=np.uint32), np.asarray(max_occupied, dtype=np.uint32),
            np.ascontiguousarray(means, dtype=f32).reshape(-1, 3))


class Result:
    """What the model wrote: statuses (per insert), pixels (per pixels op), box, and per aggregation a dict with box,
    yz, sums, counts, occupied, voxels, image."""


def _box(data, at):
    v = struct.unpack_from("<7i", data, at)
    return (None if v[0] else (np.array(v[1:4], dtype=np.int32), np.array(v[4:7], dtype=np.int32))), at + 28


def run_model(exe, voxel_size, transform, ops, directory, floors=1, timing=False):
    src, dst = os.path.join(str(directory), "xray_ops.bin"), os.path.join(str(directory), "xray_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<d7fi", voxel_size, *[float(v) for v in transform], floors))
        for o in ops:
            if o[0] == "insert":
                _, a, pts, col = o
                f.write(struct.pack("<4i", 1, a, len(pts), len(col)) + pts.tobytes() + col.tobytes())
            else:
                _, n, mx, means = o
                rec = np.zeros(len(n), dtype=[("n", "<u4"), ("m", "<u4"), ("c", "<f4", 3)])
                rec["n"], rec["m"], rec["c"] = n, mx, means
                f.write(struct.pack("<2i", 2, len(n)) + rec.tobytes())
    text = subprocess.check_output([exe, src, dst] + (["--time"] if timing else [])).decode()
    data = open(dst, "rb").read()
    r = Result()
    r.statuses, r.pixels, at = [], [], 0
    for o in ops:
        if o[0] == "insert":
            r.statuses.append(struct.unpack_from("<i", data, at)[0])
            at += 4
        else:
            r.pixels.append(np.frombuffer(data, dtype=np.uint32, count=len(o[1]), offset=at).copy())
            at += 4 * len(o[1])
    r.box, at = _box(data, at)
    r.aggregations = []
    for _ in range(floors):
        a = {}
        a["box"], at = _box(data, at)
        n = struct.unpack_from("<q", data, at)[0]
        rec = np.frombuffer(data, dtype=[("yz", "<i4", 2), ("sums", "<f4", 3), ("count", "<u4"), ("occupied", "<u4")], count=n,
                            offset=at + 8)
        at += 8 + 28 * n
        a["yz"], a["sums"], a["counts"], a["occupied"] = rec["yz"].copy(), rec["sums"].copy(), rec["count"].copy(), rec["occupied"].copy()
        n = struct.unpack_from("<q", data, at)[0]
        a["voxels"] = np.frombuffer(data, dtype=np.int32, count=3 * n, offset=at + 8).reshape(n, 3).copy()
        at += 8 + 12 * n
        w, h = struct.unpack_from("<2i", data, at)
        a["image"] = np.frombuffer(data, dtype=np.uint32, count=w * h, offset=at + 8).reshape(h, w).copy()
        at += 8 + 4 * w * h
        r.aggregations.append(a)
    assert at == len(data)
    if timing:
        words = text.split()
        r.insert_seconds, r.draw_seconds = float(words[1]), float(words[3])
    return r


def intensity_colors(intensities, lo, hi):
    """IntensityToColorPointsProcessor::Process (io/intensity_to_color_points_processor.cc:49-54) in float."""
    i = np.asarray(intensities, dtype=f32)
    gray = np.clip((i - f32(lo)) / (f32(hi) - f32(lo)), f32(0), f32(1)).astype(f32)
    return np.stack([gray, gray, gray], axis=1)


_DRIVES = {}  # a drive is made once per process


def drive_ops(num_scans, beams, azimuths, colors, seed=7):
    """The drive of outlier_common (closed cube, static and moving spheres) as inserts.  colors: "none", "constant" (one
    colour per batch, a different one each batch, as color_points gives per frame_id), "intensity" (per point, from random
    intensities through the intensity formula)."""
    rng = np.random.RandomState(seed)
    ops = []
    if (num_scans, beams, azimuths) not in _DRIVES:
        _DRIVES[(num_scans, beams, azimuths)] = oc.drive(num_scans, beams, azimuths)
    for s, (_, pts) in enumerate(_DRIVES[(num_scans, beams, azimuths)]):
        if colors == "none":
            ops.append(insert(pts))
        elif colors == "constant":
            ops.append(insert(pts, (rng.randint(0, 256, 3) / f32(255.0)).astype(f32)))
        else:
            ops.append(insert(pts, intensity_colors(rng.uniform(-20.0, 300.0, len(pts)), 0.0, 255.0)))
    return ops


def camera_cells(voxel_size, transform, pts):
    """The model's cells of `pts` in numpy float32 (for honest() only; the comparison itself never uses it)."""
    t = np.asarray(transform, dtype=f32)
    w, qx, qy, qz = t[3], t[4], t[5], t[6]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    uvx, uvy, uvz = qy * z - qz * y, qz * x - qx * z, qx * y - qy * x
    uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
    cx, cy, cz = qy * uvz - qz * uvy, qz * uvx - qx * uvz, qx * uvy - qy * uvx
    cam = np.stack([((x + w * uvx) + cx) + t[0], ((y + w * uvy) + cy) + t[1], ((z + w * uvz) + cz) + t[2]], axis=1)
    assert cam.dtype == f32
    q = cam / f32(voxel_size)
    return np.where(q >= 0, np.floor(q + f32(0.5)), np.ceil(q - f32(0.5))).astype(np.int64)


def order_sensitive_fraction(voxel_size, transform, ops):
    """Of the columns with eight or more points: the share whose sequential float32 sum, in insertion order, differs in
    bits from the sum of the same addends in reverse order (red channel).  Recomputed from the inputs in numpy; of more
    than 2000 such columns every k-th is looked at."""
    keys, reds = [], []
    for o in ops:
        if o[0] != "insert" or len(o[2]) == 0:
            continue
        cells = camera_cells(voxel_size, transform, o[2])
        keys.append(cells[:, 1] * 65536 + cells[:, 2] + o[1] * (1 << 40))
        col = o[3]
        reds.append(np.zeros(len(o[2]), dtype=f32) if len(col) == 0 else (np.full(len(o[2]), col[0, 0], dtype=f32) if len(col) == 1
                                                                         else col[:, 0]))
    keys, reds = np.concatenate(keys), np.concatenate(reds)
    order = np.argsort(keys, kind="stable")
    keys, reds = keys[order], reds[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[starts[1:], len(keys)]
    big = differ = 0
    long_enough = np.flatnonzero(ends - starts >= 8)
    long_enough = long_enough[::max(1, len(long_enough) // 2000)]
    for a, b in zip(starts[long_enough], ends[long_enough]):
        big += 1
        forward = backward = f32(0)
        for v in reds[a:b]:
            forward = f32(forward + v)
        for v in reds[a:b][::-1]:
            backward = f32(backward + v)
        differ += forward.tobytes() != backward.tobytes()
    return differ / max(big, 1), big


def honest(result, ops=None, voxel_size=None, transform=None, colored=False):
    """The conditions under which a parity case compares something, from the model's output (and, for the order of the
    sums, from the inputs)."""
    assert all(s == 0 for s in result.statuses), "a parity case may not contain a refusal"
    for a in result.aggregations:
        image = a["image"]
        assert image.shape[0] > 1 and image.shape[1] > 1, image.shape
        assert np.any(image == WHITE) and np.any(image != WHITE), "the image needs empty and occupied pixels"
    assert max(int(a["occupied"].max()) for a in result.aggregations) >= 8, "the logarithmic scale is not exercised"
    if colored:
        fraction, big = order_sensitive_fraction(voxel_size, transform, ops)
        assert big >= 10 and fraction >= 0.10, (fraction, big)
        return fraction
    return None


# ---- the device side -------------------------------------------------------------------------------------------------
def run_device(dl, ctx, voxel_size, transform, ops, floors=1, registered=False):
    """The inserts of `ops` on `floors` PointsXray objects -> (aggregators, statuses)."""
    xs = [dl.PointsXray(ctx, voxel_size, transform) for _ in range(floors)]
    statuses = []
    for o in ops:
        if o[0] != "insert":
            continue
        _, a, pts, col = o
        cloud = dl.PointCloud(ctx, pts)
        if registered and len(col) > 1:
            ctx.host_register(col)
        try:
            xs[a].insert(cloud, None if len(col) == 0 else col)
            statuses.append(0)
        except dl.DliomError as e:
            statuses.append(e.status)
        finally:
            if registered and len(col) > 1:
                ctx.host_unregister(col)
            cloud.close()
    return xs, statuses


def merged_box(xs):
    boxes = [b for b in (x.bounding_box() for x in xs) if b is not None]
    if not boxes:
        return None
    return np.min([b[0] for b in boxes], axis=0).astype(np.int32), np.max([b[1] for b in boxes], axis=0).astype(np.int32)


def assert_box_equal(got, want):
    assert (got is None) == (want is None)
    if got is not None:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)


def assert_equal(xs, statuses, result):
    """Column table (sums compared as bits), voxel list, bounding boxes and image bytes, per aggregation."""
    assert statuses == result.statuses, (statuses, result.statuses)
    box = merged_box(xs)
    assert_box_equal(box, result.box)
    for x, a in zip(xs, result.aggregations):
        assert_box_equal(x.bounding_box(), a["box"])
        yz, sums, counts, occupied = x.columns()
        assert np.array_equal(yz, a["yz"]) and np.array_equal(counts, a["counts"]) and np.array_equal(occupied, a["occupied"])
        assert sums.tobytes() == a["sums"].tobytes(), "column sums differ in bits: %d of %d columns" % (
            int(np.any(sums.view(np.uint32) != a["sums"].view(np.uint32), axis=1).sum()), len(sums))
        assert np.array_equal(x.voxels(), a["voxels"])
        image = x.draw(box)
        assert image.shape == a["image"].shape and image.tobytes() == a["image"].tobytes()
        stats = x.stats()
        assert stats["voxels"] == len(a["voxels"]) and stats["columns"] == len(a["yz"])


def compare(dl, ctx, exe, voxel_size, transform, ops, directory, floors=1, colored=False, need_honest=True, registered=False):
    result = run_model(exe, voxel_size, transform, ops, directory, floors)
    fraction = honest(result, ops, voxel_size, transform, colored) if need_honest else None
    xs, statuses = run_device(dl, ctx, voxel_size, transform, ops, floors, registered)
    try:
        assert_equal(xs, statuses, result)
        stats = [x.stats() for x in xs]
    finally:
        for x in xs:
            x.close()
    return result, stats, fraction


# ---- prescribed runs and column counts (the per-point sums' path edges and the sort's key width) ------------------------
# points_xray.hip: one lane sums a run of up to 64 points of a column, a wavefront in trips of 64 anything longer; a run goes
# to the wavefront only when a 65th point follows; the wavefront's loop ends on a trip of fewer than 64.
RUN_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 192, 193]
RUN_LAST = [64, 65, 128]  # the variants: the run that gets the highest column slot and so ends the sorted arrays
RUN_SEED = 1  # chosen on the CPU (tests/test_points_xray_host.py): every run of 64 or more is order-sensitive with it
COLUMN_COUNTS = [255, 256, 257, 65535, 65536, 65537]


def _column_point(column, x):
    """A point of column `column` (cells y = column % 256 - 128, z = column // 256 - 128) at voxel size 1, identity."""
    return [x + 0.1, column % 256 - 128 + 0.1, column // 256 - 128 - 0.1]


def run_length_batch(seed=RUN_SEED):
    """One batch whose columns 0..9 receive RUN_LENGTHS[k] points, interleaved by a fixed permutation (only a stable sort
    keeps a run in batch order), with random colours -> (points, colours, column of every point)."""
    rng = np.random.RandomState(seed)
    column = rng.permutation(np.repeat(np.arange(len(RUN_LENGTHS)), RUN_LENGTHS))
    pts = np.array([_column_point(3 * c, i % 37) for i, c in enumerate(column)], dtype=f32)
    return pts, rng.uniform(0.0, 1.0, (len(pts), 3)).astype(f32), column


def run_length_ops(last, colors="point", seed=RUN_SEED):
    """Ten one-point inserts, one a column, claim the column slots in a known order (a slot is given out per new column,
    insert after insert) with the run of `last` points last; then the batch twice: the second time the sums continue from
    the stored ones.  colors: "point", "constant" (one colour a batch) or "none"."""
    pts, col, column = run_length_batch(seed)
    order = [k for k in range(len(RUN_LENGTHS)) if RUN_LENGTHS[k] != last] + [RUN_LENGTHS.index(last)]
    rng = np.random.RandomState(seed + 1)
    ops = []
    for k in order:
        c = rng.uniform(0.0, 1.0, 3).astype(f32)
        ops.append(insert([_column_point(3 * k, 50)], None if colors == "none" else c))
    for _ in range(2):
        c = rng.uniform(0.0, 1.0, 3).astype(f32)
        ops.append(insert(pts, col if colors == "point" else (c if colors == "constant" else None)))
    return ops


def run_lengths_of(voxel_size, transform, pts):
    """The run lengths of a batch, from camera_cells, in the order of the columns' (y, z)."""
    cells = camera_cells(voxel_size, transform, pts)
    _, counts = np.unique(cells[:, 1] * 65536 + cells[:, 2], return_counts=True)
    return counts.tolist()


def order_sensitive_runs(colors, column):
    """For every run of 64 or more points: does the sequential float32 sum of its red values, in batch order, differ from
    the sum in reverse order AND from a pairwise (tree) sum?"""
    def pairwise(v):
        v = list(v)
        while len(v) > 1:
            v = [f32(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
        return v[0]
    out = []
    for k, length in enumerate(RUN_LENGTHS):
        if length < 64:
            continue
        reds = colors[column == k, 0]
        forward = backward = f32(0)
        for v in reds:
            forward = f32(forward + v)
        for v in reds[::-1]:
            backward = f32(backward + v)
        out.append(forward.tobytes() != backward.tobytes() and forward.tobytes() != pairwise(reds).tobytes())
    return out


def column_count_ops(count, colors="point"):
    """Inserts that leave the aggregator with exactly `count` columns.  A one-point insert gives column 0 slot 0; the next
    batches (of up to 40 000 points) have one point a column for the columns 1 .. count - 2 and a few repeats; the last batch brings the last column --
    the highest slot, count - 1 -- as a run of 3 with distinct colours, interleaved with points of column 0 (the slot that
    count - 1 turns into when count - 1 is a power of two and the sort drops the top key bit) and a few other columns."""
    rng = np.random.RandomState(count)

    def colours(n):
        if colors == "none":
            return None
        return rng.uniform(0.0, 1.0, (n, 3)).astype(f32) if colors == "point" else rng.uniform(0.0, 1.0, 3).astype(f32)
    first = [_column_point(c, 0) for c in range(1, count - 1)] + [_column_point(c, 1 + i) for i, c in enumerate((1, 2, 3, 2, 1, count - 2))]
    n, x = count - 1, 0
    last = [_column_point(c, i) for i, c in enumerate([n, x, n, x, n, 5, 7, 5])]
    pieces = [first[i:i + 40000] for i in range(0, len(first), 40000)]  # no batch above 65 537 points
    return ([insert([_column_point(0, 9)], colours(1))] + [insert(p, colours(len(p))) for p in pieces] + [insert(last, colours(len(last)))])
