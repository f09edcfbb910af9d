"""Shared by tests/test_voxel_table_host.py and tests/test_gpu_voxel_table.py: the export stages' voxel table
(d-liom_amd/csrc/voxel_hash.h, voxel_table.hip) under crowded hashing.

  * mirrors of hash_key, of the leaf key and of the column key, written from the header's comments;
  * colliding_leaves() / colliding_columns(): voxels whose keys' hashes share their low bits, found once per process;
  * Table: what the header promises, as a sequential program (claim, find, growth by the stated rule);
  * the cases (one chain, wrap-around, growth over a crowded chain, contention, the ray walk through a crowd) as point
    batches for the two CPU models and the device, and the probe sums the table's layout forces on every look-up.

Voxel size 0.5: a point c * 0.5 is exact in float and p / resolution is exactly c, for every c in [-8192, 8191].

The probe sums.  With linear probing the set of occupied entries does not depend on the order of the insertions, and a
key's probes are 1 + (its entry - its home entry), so the sum of the probes over all keys, each looked up once, is
(number of keys) + (sum of the occupied entries) - (sum of the home entries): the same for every order, a racing one
included.  For L keys with one home entry and nothing else in their way it is L (L + 1) / 2, and no neighbour can make it
less.  Where a key is looked up m times the look-ups cost at least m_min * (that sum) + (look-ups - m_min * keys).
test_voxel_table_host.py checks the invariance on every case; the device tests assert the bounds against `probes`."""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_common as oc  # noqa: E402
import points_xray_common as xc  # noqa: E402
from outlier_common import FILTER, MARK, RAYS, f32, op  # noqa: E402

VOXEL_SIZE = 0.5
INITIAL_CAPACITY = 1024
_M64 = (1 << 64) - 1


# ---- mirrors of voxel_hash.h ------------------------------------------------------------------------------------------
def hash_int(k):
    """hash_key of one key (a Python int)."""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    k ^= k >> 33
    return k & 0xFFFFFFFF


def hash_key(keys):
    """hash_key of an array of keys -> uint32."""
    k = np.array(keys, dtype=np.uint64, ndmin=1)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def leaf_key(voxels):
    """Three 14-bit fields of (c >> 3) + 1024, x least significant."""
    leaf = (np.asarray(voxels, dtype=np.int64).reshape(-1, 3) >> 3) + 1024
    return (leaf[:, 0] | (leaf[:, 1] << 14) | (leaf[:, 2] << 28)).astype(np.uint64)


def column_key(yz):
    """(cy + 8192) << 14 | (cz + 8192)."""
    yz = np.asarray(yz, dtype=np.int64).reshape(-1, 2)
    return (((yz[:, 0] + 8192) << 14) | (yz[:, 1] + 8192)).astype(np.uint64)


# ---- the search for colliding keys ------------------------------------------------------------------------------------
class _Domain:
    """The voxels a search looks at, numbered 0 .. 2^index_bits - 1, with the hashes of their keys (made once)."""

    def __init__(self, index_bits, coords_of, key_of, low_corner, high_corner):
        self.size, self.coords_of, self.key_of = 1 << index_bits, coords_of, key_of
        self.low_corner, self.high_corner = low_corner, high_corner  # index -> bool: the extent's first / last leaf or column
        self._hashes, self._cache = None, {}

    def hashes(self):
        if self._hashes is None:
            step = 1 << 20
            self._hashes = np.concatenate([hash_key(self.key_of(self.coords_of(np.arange(a, a + step, dtype=np.int64))))
                                           for a in range(0, self.size, step)])
        return self._hashes

    def members(self, bits, bucket):
        return np.flatnonzero((self.hashes() & np.uint32((1 << bits) - 1)) == np.uint32(bucket))

    def corner_bucket(self, bits, need):
        """The lowest bucket of `need` or more keys that holds the most kinds of corner (first, last) a bucket of that
        size holds at all."""
        key = ("bucket", bits, need)
        if key not in self._cache:
            low = (self.hashes() & np.uint32((1 << bits) - 1)).astype(np.int64)
            index = np.arange(self.size, dtype=np.int64)
            total = np.bincount(low, minlength=1 << bits)
            kinds = ((np.bincount(low[self.low_corner(index)], minlength=1 << bits) > 0).astype(np.int64) +
                     (np.bincount(low[self.high_corner(index)], minlength=1 << bits) > 0))
            kinds[total < need] = -1
            assert kinds.max() >= 0, "no bucket of %d bits holds %d keys" % (bits, need)
            self._cache[key] = int(np.argmax(kinds))
        return self._cache[key]

    def colliding(self, count, bits, bucket, seed):
        key = ("colliding", count, bits, bucket, seed)
        if key not in self._cache:
            index = self.members(bits, bucket)
            corner = self.low_corner(index) | self.high_corner(index)
            rest = index[~corner]
            chosen = np.concatenate([index[corner][:8], np.random.RandomState(seed).permutation(rest)])[:count]
            assert len(chosen) == count, "bucket %d of %d bits holds %d keys, not %d" % (bucket, bits, len(index), count)
            out = self.coords_of(chosen)
            out.setflags(write=False)
            self._cache[key] = out
        return self._cache[key]

    def ordinary(self, count, seed, avoid_bits, avoid_bucket, capacity=None, first=0, width=0):
        """`count` distinct voxels outside the bucket (avoid_bits, avoid_bucket), chosen with `seed`; with `capacity`:
        only ones whose home entry in a table of that capacity is one of the `width` entries from `first` on."""
        h = self.hashes()
        ok = (h & np.uint32((1 << avoid_bits) - 1)) != np.uint32(avoid_bucket)
        if capacity is not None:
            ok &= ((h.astype(np.int64) - first) & (capacity - 1)) < width
        index = np.flatnonzero(ok)
        return self.coords_of(np.sort(np.random.RandomState(seed).choice(index, count, replace=False)))


LEAF_SPAN = 32      # leaves: lx over the whole extent, ly and lz in [-32, 31] -- an x-ray image of 512 x 512 pixels
COLUMN_SPAN = 128   # columns: cy over the whole extent, cz in [-128, 127] -- an image of 16384 x 256 pixels


def _leaf_voxels(i):  # the centre cell 8 * l + 4 of leaf number i
    leaf = np.stack([(i & 2047) - 1024, ((i >> 11) & 63) - LEAF_SPAN, (i >> 17) - LEAF_SPAN], axis=1)
    return 8 * leaf + 4


def _columns(i):
    return np.stack([(i & 16383) - 8192, (i >> 14) - COLUMN_SPAN], axis=1)


LEAVES = _Domain(23, _leaf_voxels, leaf_key, lambda i: (i & 2047) == 0, lambda i: (i & 2047) == 2047)
COLUMNS = _Domain(22, _columns, column_key, lambda i: (i & 16383) == 0, lambda i: (i & 16383) == 16383)


def colliding_leaves(count, bits, bucket, seed=0):
    """`count` distinct voxels (int64 (count, 3), each the centre cell of its leaf) whose leaf keys' hashes have the low
    `bits` bits `bucket`; the extent's corner leaves (l = -1024, l = 1023 on x) of the bucket come first."""
    return LEAVES.colliding(count, bits, bucket, seed)


def colliding_columns(count, bits, bucket, seed=0):
    """`count` distinct columns (int64 (count, 2): cy, cz) whose column keys' hashes have the low `bits` bits `bucket`."""
    return COLUMNS.colliding(count, bits, bucket, seed)


# ---- the table as a sequential program ---------------------------------------------------------------------------------
class Table:
    """voxel_hash.h, one thread: open addressing with linear probing, the slot of a key given out at its claim and kept
    through every growth; 1024 entries at first, doubled until capacity >= 2 * want (voxel_table.hip)."""

    def __init__(self):
        self.capacity, self.growths, self.slot_key = 0, 0, []
        self.grow(INITIAL_CAPACITY // 2)

    def home(self, key):
        return hash_int(key) & (self.capacity - 1)

    def _walk(self, key):  # -> the entry that holds `key` or the free entry that ends its chain, entries read
        h, probes = self.home(key), 1
        while self.keys[h] is not None and self.keys[h] != key:
            h, probes = (h + 1) & (self.capacity - 1), probes + 1
        return h, probes

    def claim(self, key):
        h, _ = self._walk(key)
        if self.keys[h] is None:
            self.keys[h], self.slots[h] = key, len(self.slot_key)
            self.slot_key.append(key)

    def find(self, key):
        """-> (slot or None, entries read)."""
        h, probes = self._walk(key)
        return (None if self.keys[h] is None else self.slots[h]), probes

    def grow(self, want, order=None):
        """Room for `want` slots at a load of at most one half; the keys of the slots in use placed into the new table
        (in slot order, or in `order`)."""
        if 2 * want <= self.capacity:
            return
        self.growths += self.capacity > 0
        self.capacity = max(self.capacity, INITIAL_CAPACITY)
        while self.capacity < 2 * want:
            self.capacity *= 2
        self.keys, self.slots = [None] * self.capacity, [None] * self.capacity
        for s in (range(len(self.slot_key)) if order is None else order):
            h, _ = self._walk(self.slot_key[s])
            self.keys[h], self.slots[h] = self.slot_key[s], s

    def insert_batch(self, keys):
        """What a stage does with a batch of points: grow for "every point a key of its own", then claim."""
        self.grow(len(self.slot_key) + len(keys))
        for k in keys:
            self.claim(int(k))
        return self.capacity

    def occupied(self):
        return [h for h in range(self.capacity) if self.keys[h] is not None]

    def probe_sum(self, keys=None):
        """The entries read when every key (of `keys`, or of the table) is looked up once."""
        return sum(self.find(int(k))[1] for k in (self.slot_key if keys is None else keys))


def closed_form_probe_sum(table):
    """keys + (occupied entries) - (home entries), the entries numbered from a free one on so that no run of occupied
    entries passes the end of the numbering."""
    free = table.keys.index(None)
    at = lambda h: (h - free) & (table.capacity - 1)  # noqa: E731
    return len(table.slot_key) + sum(at(h) for h in table.occupied()) - sum(at(table.home(k)) for k in table.slot_key)


def lookup_bound(table, looked_up):
    """The least the look-ups of `looked_up` (one key per look-up, every key of the table at least once) can read."""
    keys, counts = np.unique(np.asarray(looked_up, dtype=np.uint64), return_counts=True)
    assert len(keys) == len(table.slot_key)
    least = int(counts.min())
    return least * table.probe_sum() + (len(looked_up) - least * len(keys))


def chain_bound(length):
    return length * (length + 1) // 2


# ---- the cases ----------------------------------------------------------------------------------------------------------
def points_of(voxels):
    return (np.asarray(voxels, dtype=np.float64).reshape(-1, 3) * VOXEL_SIZE).astype(f32)


def _with_x(columns, rng):
    """A voxel in each column (cy, cz) at a random x cell in [-64, 63]."""
    columns = np.asarray(columns).reshape(-1, 2)
    return np.concatenate([rng.randint(-64, 64, (len(columns), 1)), columns], axis=1).astype(np.int64)


def _case(name, kind, crowd, batches, rng, **more):
    """batches: voxels int64 (n, 3) each.  kind: which table the crowd sits in ("leaves": both stages, "columns": x-ray)."""
    c = types.SimpleNamespace(name=name, kind=kind, crowd=crowd, batches=batches, **more)
    c.crowd_keys = [int(k) for k in (leaf_key(crowd) if kind == "leaves" else column_key(crowd))]
    c.length = len(c.crowd_keys)
    c.colors = [rng.uniform(0.0, 1.0, (len(b), 3)).astype(f32) for b in batches]
    return c


_CASES = {}


def _cached(make):
    def wrapped(*args):
        key = (make.__name__,) + args
        if key not in _CASES:
            _CASES[key] = make(*args)
        return _CASES[key]
    return wrapped


ONE_CHAIN_COUNTS = [3, 64, 65, 70, 63, 66]  # points of the first colliding columns; the others get 3 .. 70 at random


@_cached
def one_chain(kind):
    """a. 64 keys that share their low 14 hash bits and 200 ordinary points, 50 of them with home entries from four before
    the crowd's to its end, in one batch.  kind "columns": 3 to 70 points in each colliding column, interleaved."""
    rng = np.random.RandomState(101)
    domain = LEAVES if kind == "leaves" else COLUMNS
    bucket = domain.corner_bucket(14, 80)
    if kind == "leaves":
        crowd = colliding_leaves(64, 14, bucket)
        capacity, voxels = 1024, crowd
    else:
        crowd = colliding_columns(64, 14, bucket)
        counts = np.concatenate([ONE_CHAIN_COUNTS, rng.randint(3, 71, 64 - len(ONE_CHAIN_COUNTS))])
        capacity, voxels = 8192, _with_x(np.repeat(crowd, counts, axis=0), rng)  # 2 * (points) > 4096
    far = domain.ordinary(150, 102, 14, bucket)
    near = domain.ordinary(50, 103, 14, bucket, capacity, (bucket - 4) & (capacity - 1), 68)
    others = np.concatenate([far, near])
    if kind == "columns":
        others = _with_x(others, rng)
    batch = rng.permutation(np.concatenate([voxels, others]))
    return _case("one chain", kind, crowd, [batch], rng, capacities=[capacity], others=others)


@_cached
def wrap_around(kind):
    """b. 40 keys whose home is the last entry of the 1024-entry table, and 10 whose home is entry 0 or 1."""
    rng = np.random.RandomState(111)
    find = colliding_leaves if kind == "leaves" else colliding_columns
    crowd = find(40, 10, 1023)
    behind = np.concatenate([find(5, 10, 0), find(5, 10, 1)])
    voxels = np.concatenate([crowd, behind])
    if kind == "columns":
        voxels = _with_x(voxels, rng)
    return _case("wrap-around", kind, crowd, [rng.permutation(voxels)], rng, capacities=[1024], behind=behind)


@_cached
def growth(kind):
    """c. 64 keys that share their low 16 hash bits; 3000 points in distinct leaves (columns), which take the capacity
    from 1024 to 8192 in one growth; the 64 voxels again."""
    rng = np.random.RandomState(121)
    domain = LEAVES if kind == "leaves" else COLUMNS
    bucket = domain.corner_bucket(16, 64)
    if kind == "leaves":
        crowd = colliding_leaves(64, 16, bucket)
        first, filler = crowd, domain.ordinary(3000, 122, 16, bucket)
    else:
        crowd = colliding_columns(64, 16, bucket)
        first, filler = _with_x(crowd, rng), _with_x(domain.ordinary(3000, 122, 16, bucket), rng)
    first = rng.permutation(first)
    return _case("growth", kind, crowd, [first, rng.permutation(filler), first[::-1].copy()], rng, capacities=[1024, 8192, 8192])


@_cached
def contention(kind, shuffled):
    """d. 64 keys that share their low 16 hash bits, each hit by 128 points of one batch of 8192: capacity 16384.  Not
    shuffled: a key's points are adjacent, all 64 lanes of a wave claim one key.  Shuffled: a wave holds many keys of the
    one chain.  kind "leaves": the 128 points of a key are one voxel."""
    rng = np.random.RandomState(131)
    domain = LEAVES if kind == "leaves" else COLUMNS
    bucket = domain.corner_bucket(16, 64)
    if kind == "leaves":
        crowd = colliding_leaves(64, 16, bucket)
        voxels = np.repeat(crowd, 128, axis=0)
    else:
        crowd = colliding_columns(64, 16, bucket)
        voxels = _with_x(np.repeat(crowd, 128, axis=0), rng)
    if shuffled:
        voxels = rng.permutation(voxels)
    return _case("contention", kind, crowd, [voxels], rng, capacities=[16384])


def ray_walk():
    """e. (remover) case a marked; rays from the origin to the 64 crowded points and to 2x and 3x their position where that
    is inside the extent: those pass through the crowded voxels.  -> (case a, the three clouds as voxels)"""
    a = one_chain("leaves")
    clouds = [a.crowd]
    for factor in (2, 3):
        further = a.crowd * factor
        clouds.append(further[np.all((further >= -8192) & (further <= 8191), axis=1)])
    return a, clouds


def key_function(kind):
    return leaf_key if kind == "leaves" else (lambda v: column_key(np.asarray(v)[:, 1:]))


def simulate(case, kind=None, batches=None):
    """The sequential table of `kind` (default: the one the crowd sits in) after the case's first `batches` batches (default:
    all) -> (table, capacity at every batch's launches)."""
    key_of = key_function(case.kind if kind is None else kind)
    table, capacities = Table(), []
    for b in case.batches[:batches]:
        capacities.append(table.insert_batch(key_of(b)))
    return table, capacities


def batch_lookup_bound(table, looked_up, crowd_keys):
    """The least the look-ups `looked_up` (one key each) can read in `table`, whatever order filled it.  All keys of the
    table looked up: lookup_bound().  Otherwise, if the crowd is among them and has one home entry: its chain sum and one
    entry for every other look-up.  Otherwise one entry a look-up."""
    distinct = set(int(k) for k in looked_up)
    if len(distinct) == len(table.slot_key):
        return lookup_bound(table, looked_up)
    crowd = set(crowd_keys)
    if crowd and crowd <= distinct and len({table.home(k) for k in crowd}) == 1:
        return chain_bound(len(crowd)) + len(looked_up) - len(crowd)
    return len(looked_up)


# ---- the cases as operations of the two CPU models ---------------------------------------------------------------------
ORIGIN = (0.0, 0.0, 0.0)


def short_ray(voxel):
    """A ray that looks the leaf of `voxel` (its centre cell) up once and counts nothing: from the cell before it on x to
    it, half a metre, exact in float.  x = 0 is its only sample; it lies at the ray's origin, in the same leaf, in a cell no
    case marks."""
    end = points_of([voxel])
    return op(RAYS, end, end[0] - np.array([VOXEL_SIZE, 0.0, 0.0], dtype=f32))


def remover_ops(case, short=(), ray_clouds=None, filter_clouds=None):
    """Every batch marked; a short ray to every voxel of `short`; rays from the origin to `ray_clouds` (voxels; default: one
    point per crowded voxel); every batch (and `filter_clouds`) filtered."""
    rays = [case.crowd] if ray_clouds is None else ray_clouds
    return ([op(MARK, points_of(b), ORIGIN) for b in case.batches] + [short_ray(v) for v in short] +
            [op(RAYS, points_of(r), ORIGIN) for r in rays] +
            [op(FILTER, points_of(b), ORIGIN) for b in list(case.batches) + list(filter_clouds or [])])


def xray_ops(case, colors="point"):
    return [xc.insert(points_of(b), c if colors == "point" else None) for b, c in zip(case.batches, case.colors)]


def determined(table, looked_up):
    """Every key of the table is looked up, each as often as every other: the entries read are lookup_bound() exactly."""
    keys, counts = np.unique(np.asarray(looked_up, dtype=np.uint64), return_counts=True)
    return len(keys) == len(table.slot_key) and counts.min() == counts.max()


def remover_probe_bound(case, ray_ends):
    """The least the remover's rays to `ray_ends` can read (voxels, each the centre cell of its leaf: a ray's last samples
    lie within one voxel of its end, so its leaf is looked up) -> (bound, whether short rays to them read exactly that)."""
    ray_ends = np.asarray(ray_ends).reshape(-1, 3)
    assert np.all((ray_ends & 7) == 4)
    table = simulate(case, "leaves")[0]
    return batch_lookup_bound(table, leaf_key(ray_ends), case.crowd_keys), determined(table, leaf_key(ray_ends))


def xray_probe_bound(case):
    """The least `probes` of the x-ray can be after the case: the mark kernel looks every point of a batch up in both
    tables as they are after that batch -> (bound, whether `probes` is exactly that)."""
    total, exact = 0, True
    for kind in ("leaves", "columns"):
        for i, b in enumerate(case.batches):
            table, _ = simulate(case, kind, i + 1)
            total += batch_lookup_bound(table, key_function(kind)(b), case.crowd_keys if kind == case.kind else [])
            exact = exact and determined(table, key_function(kind)(b))
    return total, exact


REMOVER_CASES = ["one_chain", "wrap_around", "growth", "contention_adjacent", "contention_shuffled", "ray_walk"]


def remover_case(name):
    """-> (case, the voxels short rays go to, the clouds rays from the origin are counted to, further clouds to filter), all as
    voxels.  The short rays and the first ray cloud end in centre cells of leaves, every crowded one among them:
    remover_probe_bound() is about them."""
    if name == "ray_walk":
        a, clouds = ray_walk()
        return a, a.crowd[:0], clouds, clouds[1:]
    case = {"one_chain": lambda: one_chain("leaves"), "wrap_around": lambda: wrap_around("leaves"),
            "growth": lambda: growth("leaves"), "contention_adjacent": lambda: contention("leaves", False),
            "contention_shuffled": lambda: contention("leaves", True)}[name]()
    if name == "growth":  # 3064 leaves: the crowd alone
        return case, case.crowd, [case.crowd], []
    every = np.unique(np.concatenate(case.batches), axis=0)  # every key of the table is looked up
    return case, every, [every if name in ("one_chain", "wrap_around") else case.crowd], []
