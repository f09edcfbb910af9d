"""Inputs and the test-side model for the voxel filter tests (tests/test_gpu_voxel_filter.py on the device,
tests/test_voxel_filter_host.py without one, tools/fuzz_voxel_filter.py): the cloud builders, and a restatement of the
adaptive filter's search (sensor/internal/voxel_filter.cc:28-77) that names the PATH the search takes, so that a sweep of
`min_num_points` can be shown to reach every path before a device result is compared with anything.  Everything here runs
on the CPU oracle alone."""
import functools

import numpy as np

f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# (a) sizes: around the workgroup shapes (256 per flag / compact workgroup, 1024 per insert workgroup with a 2048-entry
# LDS table), table_capacity's steps (powers of two >= 2 n), and above 65 536 points, where a thread of the compaction
# sums more than one preceding workgroup (from workgroup 257 on)
SIZES_N = [255, 256, 257, 1023, 1024, 1025, 2047, 2049, 32768, 32769, 65535, 65537, 65793, 131073, 262145]
SIZES_EDGE = [0.05, 2.0]  # most points survive: large compaction offsets / few voxels: every workgroup meets every voxel


@functools.lru_cache(maxsize=None)
def uniform_cloud(n, size):
    """test_device_voxel_filter_equals_oracle's cloud: uniform in +-20 m, every fifth point rounded to 0.1 (duplicates
    and lattice points), every seventh on (k + 0.5) * size (the half-way cases of the rounding)."""
    rng = np.random.RandomState(n + int(size * 100))
    pts = rng.uniform(-20, 20, size=(n, 3)).astype(f32)
    pts[::5] = pts[::5].round(1)
    pts[1::7] = (np.floor(pts[1::7] / size) + 0.5) * f32(size)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def uniform_keep(orc, n, size):
    """Indices the reference keeps of uniform_cloud(n, size) (computed once, shared, read-only)."""
    keep = orc.voxel_filter(size, uniform_cloud(n, size))
    keep.setflags(write=False)
    return keep


def has_late_survivors(n, size):
    """Does uniform_cloud(n, size) have survivors at indices >= 65 536?  Every cloud larger than that at 0.05 m; at 2.0 m
    only the two largest (tests/test_voxel_filter_host.py checks this table against the oracle)."""
    return n > 65536 and (size == 0.05 or n >= 131073)


# ---------------------------------------------------------------------------------------------------------------------
# (b) clustered clouds.  Voxels of edge CLUSTER_EDGE; A is the voxel of the origin, B the voxel of CLUSTER_B.
CLUSTER_EDGE = 0.5
CLUSTER_B = np.array([3.0, -1.5, 0.5], f32)  # a voxel centre: (6, -3, 1) edges
CLUSTER_N = [5000, 70001]
B_FIRST_AT = [1023, 1024, 1025, 65536]  # last point of the first insert workgroup, first of the second, ..., of block 257


def _inside(rng, n, centre):
    """n points strictly inside the voxel around `centre` (|offset| <= 0.24 of a 0.5 edge)."""
    return (np.asarray(centre, f32) + rng.uniform(-0.24, 0.24, size=(n, 3)).astype(f32)).astype(f32)


def cluster_cases(n):
    """The names of the clustered clouds that exist at n points (a first member at index f needs n > f)."""
    names = ["one_voxel", "alternating", "b_last", "copies", "signed_zero_subnormal"]
    return names + ["b_first_at_%d" % f for f in B_FIRST_AT if f < n]


@functools.lru_cache(maxsize=None)
def cluster_cloud(name, n):
    """-> (points, the indices that survive VoxelFilter(CLUSTER_EDGE), worked out from how the cloud is built)."""
    rng = np.random.RandomState(len(name) * 1000003 + n)
    a = _inside(rng, n, (0, 0, 0))
    b = _inside(rng, n, CLUSTER_B)
    if name == "one_voxel":
        pts, keep = a, [0]
    elif name == "alternating":
        pts = a.copy()
        pts[1::2] = b[1::2]
        keep = [0, 1]
    elif name == "b_last":
        pts = a.copy()
        pts[-1] = b[-1]
        keep = [0, n - 1]
    elif name.startswith("b_first_at_"):
        first = int(name[len("b_first_at_"):])
        pts = a.copy()
        members = np.arange(first, n, 256)  # one in every flag / compact workgroup and every insert workgroup after it
        pts[members] = b[members]
        keep = [0, first]
    elif name == "copies":
        pts = np.tile(a[:1], (n, 1))  # bit-identical copies of one point
        keep = [0]
    elif name == "signed_zero_subnormal":
        # voxel A holds -0.0, 0.0, subnormals and the smallest normals of both signs on every axis (its first point is
        # all -0.0, the second all 0.0); every seventh point is B's centre with ONE coordinate replaced by such a value:
        # three more voxels, (0, -3, 1), (6, 0, 1) and (6, -3, 0), by the point's index modulo 3
        values = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38], f32)
        pts = values[rng.randint(0, len(values), size=(n, 3))]
        pts[0] = f32(-0.0)
        pts[1] = f32(0.0)
        others = np.arange(3, n, 7)
        pts[others] = CLUSTER_B
        pts[others, others % 3] = values[others % len(values)]
        keep = [0, 3, 10, 17]  # 3 % 3 = 0, 10 % 3 = 1, 17 % 3 = 2
    else:
        raise ValueError(name)
    pts = np.ascontiguousarray(pts, f32)
    pts.setflags(write=False)
    return pts, np.array(keep, np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the adaptive search.  voxel_filter.cc:28-77 restated in float32 on survivor COUNTS.
SEARCH_MAX_LENGTHS = [2.0, 0.7, 3.1]
SEARCH_MAX_RANGES = [50.0, 12.0]
MIN_DISTINCT_PATHS = {2.0: 30, 0.7: 15, 3.1: 30}


@functools.lru_cache(maxsize=None)
def search_cloud():
    """An 8 x 512 scan (4096 points) plus bit-identical copies of its first 64 points: with the copies no edge length
    keeps every point, so a threshold of n is "no length dense enough" and not "already sparse".  (Eight beams and not
    sixteen of 256 azimuths: within 12 m the 16 x 256 scan of this pose has 221 points and its sweep at max_length 2.0
    reaches 29 distinct paths, one short of MIN_DISTINCT_PATHS; this one reaches 33 there and more everywhere else.)"""
    from dliom import synth
    pts, _ = synth.scan(synth.trajectory_pose(0.3), 8, 512)
    assert len(pts) == 4096
    pts = np.ascontiguousarray(np.concatenate([pts, pts[:64]]), f32)
    pts.setflags(write=False)
    return pts


def crop(pts, max_range):
    """FilterByMaxRange (:28-37): norm() <= max_range in float, Eigen's reduction order x*x + (y*y + z*z)."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.sqrt((x * x + (y * y + z * z)).astype(f32)).astype(f32)
        return np.ascontiguousarray(pts[norm <= f32(max_range)])


class Counter:
    """Survivor counts of VoxelFilter(length) over one cropped cloud, each length filtered once."""

    def __init__(self, orc, pts, max_range):
        self.orc = orc
        self.cropped = crop(pts, max_range)
        self.n = len(self.cropped)
        self._counts = {}

    def __call__(self, length):
        key = f32(length).tobytes()
        if key not in self._counts:
            self._counts[key] = len(self.orc.voxel_filter(float(f32(length)), self.cropped)) if self.n else 0
        return self._counts[key]


def search_path(count, n, max_length, min_num_points):
    """AdaptivelyVoxelFiltered (:39-77) on counts.  -> (path, survivors).  path: "sparse" (:42-45), "max" (:46-50),
    "none" (no halving dense enough: the last one's result stands), or "<d>/<steps>": low_length = max_length / d was the
    first dense-enough halving (d = 2, 4, ..., 128) and the bisection then took `steps`, one letter per mid_length tried:
    'o' it was dense enough (low = mid), 'f' it was not (high = mid)."""
    max_length, min_points = f32(max_length), f32(min_num_points)
    if f32(n) <= min_points:
        return "sparse", n
    result = count(max_length)
    if f32(result) >= min_points:
        return "max", result
    high, divisor = max_length, 1
    while high > f32(1e-2) * max_length:
        low = high / f32(2)
        divisor *= 2
        result = count(low)
        if f32(result) >= min_points:
            steps = ""
            while (high - low) / low > f32(1e-1):
                mid = (low + high) / f32(2)
                candidate = count(mid)
                if f32(candidate) >= min_points:
                    low, result = mid, candidate
                    steps += "o"
                else:
                    high = mid
                    steps += "f"
            return "%d/%s" % (divisor, steps), result
        high = high / f32(2)
    return "none", result


def path_divisor(path):
    return int(path.split("/")[0]) if "/" in path else 0


def path_steps(path):
    return path.split("/")[1] if "/" in path else ""


def sweep_thresholds(count, n_all, max_length):
    """min_num_points values that turn every comparison of the search both ways: the counts c at a ladder of lengths
    (max_length / 2^k * (1 + j / 16), k = 1..7, j = 0..16, and max_length) -- c is the tie the `>=` turns on -- and
    c + 1; 1; the cloud's size and the cropped cloud's, and one more than each (the `<=` of "already sparse")."""
    lengths = [f32(max_length)]
    for k in range(1, 8):
        for j in range(17):
            lengths.append(f32(f32(max_length) / f32(2 ** k) * f32(1.0 + j / 16.0)))
    values = {1, n_all, n_all + 1, count.n, count.n + 1}
    for length in lengths:
        c = count(length)
        values.update((c, c + 1))
    return sorted(v for v in values if v >= 1)


@functools.lru_cache(maxsize=None)
def search_sweep(orc, max_length, max_range):
    """-> [(min_num_points, path, survivors, the oracle's AdaptiveVoxelFilter output)] over sweep_thresholds, computed
    once per (max_length, max_range) and shared."""
    pts = search_cloud()
    count = Counter(orc, pts, max_range)
    out = []
    for t in sweep_thresholds(count, len(pts), max_length):
        path, survivors = search_path(count, count.n, max_length, t)
        want = orc.adaptive_voxel_filter(max_length, t, max_range, pts)
        want.setflags(write=False)
        out.append((t, path, survivors, want))
    return out


def check_sweep_conditions(sweep, max_length):
    """What a sweep has to reach for the device comparison to mean anything (asserted on the CPU and on the GPU)."""
    paths = {path for _, path, _, _ in sweep}
    for t, path, survivors, want in sweep:
        assert survivors == len(want), (max_length, t, path, survivors, len(want))
    assert {"sparse", "max", "none"} <= paths, paths
    if max_length in (2.0, 3.1):
        # decided at max_length / 8 or below: the second insert launch, then a bisection over its table
        assert any(path_divisor(p) >= 8 for p in paths), paths
    assert max(len(path_steps(p)) for p in paths) >= 4, paths
    assert len(paths) >= MIN_DISTINCT_PATHS[max_length], (max_length, len(paths), sorted(paths))
    return paths


def pair_classes(orc):
    """One threshold per class of path, all at max_length 2.0 and max_range 50: -> {class: (max_length, min_num_points,
    max_range)}.  "first" is decided by a halving of the first insert launch and bisected, "second" by one of the second
    launch and bisected, "deepest" takes the most bisection steps."""
    sweep = search_sweep(orc, 2.0, 50.0)
    pick = {}
    for t, path, _, _ in sweep:
        d, steps = path_divisor(path), path_steps(path)
        if path in ("sparse", "max", "none"):
            pick.setdefault(path, t)
        elif steps:
            pick.setdefault("first" if d <= 4 else "second", t)
    deepest = max(sweep, key=lambda e: (len(path_steps(e[1])), path_divisor(e[1])))
    assert len(path_steps(deepest[1])) >= 4
    pick["deepest"] = deepest[0]
    assert set(pick) == {"sparse", "max", "none", "first", "second", "deepest"}, pick
    return {name: (2.0, float(t), 50.0) for name, t in pick.items()}


def sweep_entry(orc, options):
    """The oracle's output for an option triple that is part of a sweep (shared), else computed."""
    max_length, t, max_range = options
    if max_length in SEARCH_MAX_LENGTHS and max_range in SEARCH_MAX_RANGES:
        for tt, _, _, want in search_sweep(orc, max_length, max_range):
            if tt == t:
                return want
    return orc.adaptive_voxel_filter(max_length, t, max_range, search_cloud())


def cross_pairs(orc):
    """Pairs across different max_length and max_range: bisected paths of every combination's sweep, the deepest of
    each, so that the second filter's nodes sit behind a full first tree."""
    picks = []
    for max_length, max_range in ((3.1, 50.0), (0.7, 12.0), (3.1, 12.0), (0.7, 50.0), (2.0, 12.0)):
        sweep = search_sweep(orc, max_length, max_range)
        t = max(sweep, key=lambda e: (len(path_steps(e[1])), path_divisor(e[1])))[0]
        picks.append((max_length, float(t), max_range))
    classes = pair_classes(orc)
    pairs = [(picks[0], picks[1]), (picks[1], picks[2]), (picks[2], picks[3]), (picks[3], picks[4]), (picks[4], picks[0])]
    pairs += [(classes["second"], picks[0]), (picks[2], classes["none"]), (classes["sparse"], picks[1]),
              (picks[3], classes["deepest"])]
    return pairs


# ---------------------------------------------------------------------------------------------------------------------
# (c) points the adaptive filter has to drop before it rounds them
def with_unroundable_points(pts, max_range):
    """`pts` with non-finite points, and finite ones far outside any voxel key, put at the front, inside and at the end:
    all of them fail `norm <= max_range`.  -> (cloud, mask of the points that were added)."""
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 1],
                    [1e30, 0, 0], [0, -3e38, 0], [3e6, 3e6, 3e6], [0, 0, -1e9], [max_range * 1.01, 0, 0]], f32)
    at = [0, 0, 1, len(pts) // 3, len(pts) // 3, len(pts) // 2, len(pts) - 1, len(pts), len(pts), len(pts)]
    cloud = np.insert(pts, at, bad, axis=0).astype(f32)
    added = np.insert(np.zeros(len(pts), bool), at, True)
    assert len(cloud) == len(pts) + len(bad) and added.sum() == len(bad)
    return np.ascontiguousarray(cloud), added


# ---------------------------------------------------------------------------------------------------------------------
# (f) one context, changing shapes
def sequence_steps(orc):
    """[(kind, arguments)] of the scratch-reuse sequence: plain filters of very different sizes around an adaptive pair."""
    classes = pair_classes(orc)
    return [("plain", (262145, 0.05)), ("plain", (257, 2.0)), ("pair", (classes["deepest"], classes["second"])),
            ("plain", (65793, 0.05)), ("plain", (1, 0.05)), ("plain", (0, 0.05))]


def sequence_cloud(n, size):
    return uniform_cloud(n, size) if n > 0 else np.zeros((0, 3), f32)
