"""Two range sensors' clouds merged on the device: a numpy model of dliom.h's statement (StampRangeData, the overlap search,
the re-basing and the merge of mapping/internal/3d/range_data_synchronizer.cc:29-130), inputs full of equal times, and
helpers to put arrays on the device as dliom_timed_cloud objects.

Equal times are ordered by oracle.std_sort_order, the real std::sort on (key, index) pairs compared by key: the order
introsort leaves depends on the comparisons alone, not on the size of the records it moves."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
UTS_EPOCH_OFFSET_SECONDS = 719162 * 24 * 60 * 60
VELODYNE, OTHER, FLOAT32 = 1, 3, 7  # dliom_point_cloud2_mode, DLIOM_POINT_FIELD_FLOAT32
PRIMARY_TIME = (1_790_000_000 + UTS_EPOCH_OFFSET_SECONDS) * 10 ** 7  # ticks of a stamp of this decade


def seconds(ticks):
    """common::ToSecondsStamp of universal-time ticks, as the adapter's Seconds()"""
    return f64(int((int(ticks) - UTS_EPOCH_OFFSET_SECONDS * 10 ** 7) * 100)) * f64(1e-9)


def stamp(xyzt, scan_period):
    out = np.array(xyzt, f32).reshape(-1, 4).copy()
    n = len(out)
    if n < 2:
        return out
    duration = f64(scan_period) / f64(n - 1)
    out[:, 3] = (-f64(scan_period) + np.arange(n, dtype=f64) * duration).astype(f32)  # (numpy does not fuse)
    out[-1, 3] = 0
    return out


def overlap(primary_times, primary_time, secondary, secondary_time):
    """-> (i_start, i_end + 1, current_end, st), or None where the reference's CHECK(i_start != -1) fails"""
    ce = seconds(primary_time)
    cs = ce + f64(primary_times[0, 3]) if len(primary_times) else ce
    st = seconds(secondary_time)
    t = st + secondary[:, 3].astype(f64)
    inside = (t >= cs) & (t <= ce)
    if not inside.any():
        return None
    i_start = int(np.argmax(inside))
    behind = np.nonzero(t[i_start + 1:] > ce)[0]
    i_end1 = i_start + 1 + int(behind[0]) if len(behind) else len(secondary)
    return i_start, i_end1, ce, st


def merge(orc, primary, primary_time, secondary, secondary_time, primary_for_times=None):
    """-> (xyzt (m, 4), origin index float32 (m,)) in std::sort's order, or None (refused)"""
    primary = np.asarray(primary, f32).reshape(-1, 4)
    secondary = np.asarray(secondary, f32).reshape(-1, 4)
    found = overlap(primary if primary_for_times is None else primary_for_times, primary_time, secondary, secondary_time)
    if found is None:
        return None
    i_start, i_end1, ce, st = found
    part = secondary[i_start:i_end1].copy()
    part[:, 3] = ((part[:, 3].astype(f64) + st) - ce).astype(f32)
    merged = np.concatenate([primary, part])
    origin = np.concatenate([np.zeros(len(primary), f32), np.ones(len(part), f32)])
    order = orc.std_sort_order(merged[:, 3])
    return merged[order], origin[order]


# ---- inputs -----------------------------------------------------------------------------------------------------------
PATTERNS = ("distinct", "runs of 64", "all equal")


def times(pattern, n, run=64):
    """n times of one sweep, ascending, the last one 0"""
    if pattern == "all equal" or n <= 1:
        return np.zeros(n, f32)
    if pattern == "distinct":
        t = np.linspace(-0.1, 0.0, n).astype(f32)
    else:
        columns = (n + run - 1) // run
        t = np.repeat(np.linspace(-0.1, 0.0, max(columns, 2))[:columns], run)[:n].astype(f32)
    t[-1] = 0
    return t


def points(seed, t):
    rng = np.random.RandomState(seed)
    xyzt = rng.uniform(-30, 30, (len(t), 4)).astype(f32)
    xyzt[:, 3] = t
    return xyzt


def pair_of_merged_size(seed, m, pattern):
    """(primary, primary_time, secondary, secondary_time) whose merge has m points: the secondary's sweep ends half a sweep
    behind the primary's, so its second half lies outside the window ("all equal": t = 0 everywhere, the same stamp)"""
    if pattern == "all equal":
        n_s = m // 2
        secondary, secondary_time = points(seed + 1, times(pattern, n_s)), PRIMARY_TIME
        count = n_s
    else:
        n_s = max(m - m // 3, 2)
        secondary, secondary_time = points(seed + 1, times(pattern, n_s)), PRIMARY_TIME + 500_000
        window = points(0, np.array([-0.1, 0], f32))  # (the primary's first t is -0.1 whatever its size)
        i_start, i_end1, _, _ = overlap(window, PRIMARY_TIME, secondary, secondary_time)
        count = i_end1 - i_start
    assert 0 < count < m
    primary = points(seed, times(pattern, m - count))
    return primary, PRIMARY_TIME, secondary, secondary_time


# ---- arrays as device objects -------------------------------------------------------------------------------------------
def upload(dl, ctx, xyzt):
    """xyzt (n, 4) float32 -> dl.TimedCloud holding exactly these bits: a message of 16-byte records decoded in the Velodyne
    mode, whose t_i = float(double(time_i) - double(time_last)) is time_i when the last one is 0 (or, when every t is 0,
    in the untimed mode)"""
    xyzt = np.ascontiguousarray(xyzt, f32).reshape(-1, 4)
    n = len(xyzt)
    fields = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1)]
    if n and np.any(xyzt[:, 3] != 0):
        assert xyzt[-1, 3] == 0
        fields.append(("time", 12, FLOAT32, 1))
        mode = VELODYNE
    else:
        mode = OTHER
    message = dl.PointCloud2(1, n, 16, 16 * n, fields, xyzt.view(np.uint8).reshape(-1))
    cloud, _, _ = message.decode(ctx, mode)
    assert len(cloud) == n
    return cloud


def sort_keys_file(path, arrays):
    """key arrays in tests/cpp/big_sort_worklist_model.cc's format: n, then n floats as hex words"""
    with open(path, "w") as f:
        for keys in arrays:
            words = np.ascontiguousarray(keys, f32).view(np.uint32)
            f.write("%d\n%s\n" % (len(words), " ".join("%x" % w for w in words)))
