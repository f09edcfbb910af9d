"""CPU models of the approximate voxel grid (include/dliom.h, dliom_cloud_approximate_voxel_filter): the sequential loop
of the definition in numpy float32, and the parallel restatement the device runs (csrc/approx_voxel.hip) -- 512 slots as
independent streams -- so that the two can be compared without a device (tests/test_approx_voxel_host.py)."""
import numpy as np

SLOTS = 512


def voxels_and_slots(points, leaf):
    """(n, 3) int64 voxel indices (floor(p * inv) in float) and (n,) slots, the hash in wrapping 32-bit arithmetic"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    inv = np.float32(1.0) / np.float32(leaf)
    f = np.floor(p * inv)  # float32 * float32, rounded once
    if not np.isfinite(p).all() or (f < -2.0 ** 31).any() or (f >= 2.0 ** 31).any():
        raise ValueError("the definition refuses this cloud")
    v = f.astype(np.int64)
    h = (v[:, 0] * 7171 + v[:, 1] * 3079 + v[:, 2] * 4231) & 0xFFFFFFFF  # the low 32 bits are those of int arithmetic
    return p, v, (h & (SLOTS - 1)).astype(np.int64)


def sequential(points, leaf):
    """The loop of the definition, one point at a time"""
    p, v, slot = voxels_and_slots(points, leaf)
    zero = np.float32(0)
    held = {}  # slot -> [voxel, sx, sy, sz, count]
    out = []

    def flush(e):
        c = np.float32(e[4])
        out.append((e[1] / c, e[2] / c, e[3] / c))

    voxel = [tuple(r) for r in v.tolist()]
    for i in range(len(p)):
        e = held.get(slot[i])
        if e is not None and e[0] != voxel[i]:
            flush(e)
            e = None
        if e is None:
            e = held[slot[i]] = [voxel[i], zero, zero, zero, 0]
        e[1], e[2], e[3], e[4] = e[1] + p[i, 0], e[2] + p[i, 1], e[3] + p[i, 2], e[4] + 1
    for s in sorted(held):
        flush(held[s])
    return np.array(out, np.float32).reshape(-1, 3)


def parallel(points, leaf):
    """The device's replay: a stable sort by slot; run starts; a run start that is not the first of its slot evicts the run
    before it, whose output number is the exclusive count of evicting points in stream order; a slot's last run goes to
    E + the slot's rank among the occupied ones; a run's sums are taken in stream order from +0.0"""
    p, v, slot = voxels_and_slots(points, leaf)
    n = len(p)
    if n == 0:
        return np.zeros((0, 3), np.float32)
    order = np.argsort(slot, kind="stable")
    s_slot, s_voxel = slot[order], v[order]
    first_of_slot = np.r_[True, s_slot[1:] != s_slot[:-1]]
    starts = first_of_slot | np.r_[True, (s_voxel[1:] != s_voxel[:-1]).any(axis=1)]
    evicts = np.zeros(n, np.int64)
    evicts[order] = starts & ~first_of_slot  # in stream order
    exclusive = np.cumsum(evicts) - evicts
    evictions = int(evicts.sum())
    rank = np.cumsum(first_of_slot) - 1  # of the slot a sorted position lies in
    run_first = np.flatnonzero(starts)
    run_end = np.r_[run_first[1:], n]
    out = np.zeros((evictions + int(first_of_slot.sum()), 3), np.float32)
    written = np.zeros(len(out), bool)
    for a, b in zip(run_first, run_end):
        evicted = b < n and s_slot[b] == s_slot[a]
        at = exclusive[order[b]] if evicted else evictions + rank[a]
        sums = np.cumsum(np.vstack([np.zeros((1, 3), np.float32), p[order[a:b]]]), axis=0, dtype=np.float32)[-1]  # sequential
        out[at] = sums / np.float32(b - a)
        assert not written[at]
        written[at] = True
    assert written.all()
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the clouds of the tests -------------------------------------------------------------------------------------------
def colliding_pair(leaf=0.2):
    """Centres of the voxels (3, 4, 5) and (3 + 512, 4, 5): 512 * 7171 is a multiple of 512, so they share a slot"""
    a = (np.array([3.5, 4.5, 5.5]) * leaf).astype(np.float32)
    b = (np.array([515.5, 4.5, 5.5]) * leaf).astype(np.float32)
    return a, b


def alternating(n=100, leaf=0.2):
    """a b a b ...: every point evicts, n centroids from n points"""
    a, b = colliding_pair(leaf)
    rng = np.random.RandomState(11)
    cloud = np.where((np.arange(n) % 2 == 0)[:, None], a, b) + (0.3 * leaf * rng.uniform(-1, 1, (n, 3))).astype(np.float32)
    return cloud.astype(np.float32)


def a_b_a(leaf=0.2):
    """Three runs in one slot, A B A: A is emitted twice"""
    a, b = colliding_pair(leaf)
    rng = np.random.RandomState(12)
    jitter = lambda m: (0.3 * leaf * rng.uniform(-1, 1, (m, 3))).astype(np.float32)
    return np.concatenate([a + jitter(5), b + jitter(3), a + jitter(4)]).astype(np.float32)


def every_slot(leaf=0.2, shuffled=True):
    """Two points in each of the voxels (k, 0, 0), k = 0 .. 511: 7171 is odd, so they fill the 512 slots"""
    rng = np.random.RandomState(13)
    k = np.arange(SLOTS)
    cloud = np.c_[(k + 0.5) * leaf, np.full(SLOTS, 0.5 * leaf), np.full(SLOTS, 0.5 * leaf)].astype(np.float32)
    cloud = np.concatenate([cloud, cloud + np.float32(0.1 * leaf)])  # two points a voxel
    return cloud[rng.permutation(len(cloud))] if shuffled else cloud


def one_voxel(n=4097, leaf=0.2):
    rng = np.random.RandomState(14)
    return ((np.array([7.5, -3.5, 2.5]) + 0.45 * rng.uniform(-1, 1, (n, 3))) * leaf).astype(np.float32)


def random_cloud(n, seed, scale=3.0, clustered=False):
    rng = np.random.RandomState(seed)
    if clustered:
        centres = rng.uniform(-scale, scale, (max(n // 200, 1), 3))
        return (centres[rng.randint(len(centres), size=n)] + 0.05 * scale * rng.standard_normal((n, 3))).astype(np.float32)
    return rng.uniform(-scale, scale, (n, 3)).astype(np.float32)


def faces(leaf):
    """Points on voxel faces and one ulp either side, negative coordinates included"""
    k = np.arange(-6, 7)
    on = (k * np.float64(leaf)).astype(np.float32)
    near = np.concatenate([on, np.nextafter(on, np.float32(-1e9)), np.nextafter(on, np.float32(1e9)), -on])
    rng = np.random.RandomState(15)
    cloud = np.stack([near[rng.randint(len(near), size=600)] for _ in range(3)], axis=1)
    return cloud.astype(np.float32)


def wrapping(leaf=0.2):
    """Voxel indices near +-2^30 on every axis, where ix * 7171 wraps in 32 bits; floats there are 16 m apart, so the
    points are made from indices"""
    rng = np.random.RandomState(16)
    index = np.concatenate([2 ** 30 + rng.randint(-40, 40, (200, 3)) * 64, -2 ** 30 + rng.randint(-40, 40, (200, 3)) * 64])
    cloud = ((index + 0.5) * np.float64(leaf)).astype(np.float32)
    return cloud[rng.permutation(len(cloud))]
