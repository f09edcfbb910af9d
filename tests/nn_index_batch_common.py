"""What tests/test_gpu_nn_index_batch.py and tests/test_nn_index_batch_host.py share: the zoo of small target clouds, the
CPU model of an index's grid (the box of the finite points and nn_choose_grid, include/dliom.h dliom_nn_index_options),
the query sets, and the Python statement of dliom_nn_index_create_batch's schedule that the device's statistics are held
against."""
import math

import numpy as np

DEFAULT_MAX_INDICES, DEFAULT_MAX_POINTS, DEFAULT_MAX_CELLS = 64, 64 * 64 * 1024, 1 << 26
MAX_CELLS_PER_AXIS, MAX_CELLS = 1024, 1 << 22
EDGES = (0.0, 0.37, 1e-6)  # automatic; a given one; one that is grown to the 2^22-cell cap


def cloud_of_size(n, seed):
    """n points over a 6 x 4 x 2 box, two of them not finite from 16 points on"""
    rng = np.random.RandomState(seed)
    p = rng.uniform([-1.0, 0.0, 0.0], [5.0, 4.0, 2.0], (n, 3)).astype(np.float32)
    if n >= 16:
        p[n // 2] = [np.nan, 0.5, 0.5]
        p[n // 3] = [0.5, np.inf, 0.5]
    return p


def _zoo():
    z = {}
    z["p1"] = np.array([[0.25, -1.5, 3.0]], np.float32)
    z["same2"] = np.array([[1.5, 2.5, -0.5], [1.5, 2.5, -0.5]], np.float32)  # extent 0: the one-cell grid with inv = 0
    z["none"] = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    rng = np.random.RandomState(2)
    z["line"] = np.c_[rng.uniform(-3.0, 7.0, 300), np.full(300, 1.25), np.full(300, -0.5)].astype(np.float32)  # one axis has extent
    z["plane"] = np.c_[rng.uniform(-2.0, 2.0, (400, 2)), np.full(400, 0.75)].astype(np.float32)  # two axes
    for k, n in enumerate((255, 256, 257, 2049)):
        z["n%d" % n] = cloud_of_size(n, 10 + k)
    mixed = rng.uniform(-1.0, 1.0, (120, 3)).astype(np.float32)
    mixed[::7, 0] = np.nan
    mixed[3::11, 1] = np.inf
    mixed[5::13, 2] = -np.inf
    mixed[0] = [np.nan, np.inf, -np.inf]
    z["mixed"] = mixed
    lattice = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    z["lattice"] = np.concatenate([lattice, lattice[::2], lattice[::3]])[rng.permutation(60 + 30 + 20)]  # ties go to the lowest index
    near = rng.uniform(-1.0, 1.0, (150, 3))
    z["far"] = np.concatenate([near, near[:90] + [10000.0, 0.0, 0.0]]).astype(np.float32)  # the automatic edge grows by its 1.26 steps
    corners = np.array([[0.0, 0.0, 0.0], [3.0, 2.0, 1.0]], np.float32)
    for name, seed in (("twin_a", 31), ("twin_b", 32)):  # equal length, equal box, neighbours in the zoo: a slot mix-up shows
        inner = np.random.RandomState(seed).uniform([0.0, 0.0, 0.0], [3.0, 2.0, 1.0], (198, 3)).astype(np.float32)
        z[name] = np.concatenate([inner[:77], corners, inner[77:]])
    for v in z.values():
        v.setflags(write=False)
    return z


ZOO = _zoo()
NAMES = list(ZOO)  # 14 clouds


def first_k(k):
    """the first k names of the zoo, going round it again beyond its end"""
    return [NAMES[i % len(NAMES)] for i in range(k)]


# ---- the grid (d-liom_amd/csrc/nn_index_internal.h nn_set_grid, nn_choose_grid) --------------------------------------------------
def choose_grid(extent, n, edge0):
    """-> (dims, inv float32, edge float)"""
    one = ([1, 1, 1], np.float32(0.0), 0.0)
    if not all(math.isfinite(e) for e in extent):
        return one
    positive = [e for e in extent if e > 0.0]
    product = 1.0
    for e in positive:
        product *= e
    if not positive or not math.isfinite(product):
        return one
    e = edge0 if edge0 > 0.0 else 0.5 * math.pow(product / float(max(n, 1)), 1.0 / len(positive))
    if not e >= 1e-6:
        e = 1e-6
    for _ in range(400):
        with np.errstate(over="ignore"):
            f = np.float32(1.0 / e)
        if f > 0 and np.isfinite(f):
            along = [math.floor(x * float(f)) + 1.0 for x in extent]
            if all(a <= MAX_CELLS_PER_AXIS for a in along) and along[0] * along[1] * along[2] <= MAX_CELLS:
                return [int(a) for a in along], f, 1.0 / float(f)
        e *= 1.26
    return one


_GRIDS = {}


def model(name, edge0=0.0):
    """the index of a zoo cloud as the header states it: points, finite_points, lo, hi, dims, cells, cell_edge (shared)"""
    if (name, edge0) not in _GRIDS:
        p = ZOO[name]
        finite = p[np.isfinite(p).all(axis=1)]
        lo = finite.min(axis=0) if len(finite) else np.zeros(3, np.float32)
        hi = finite.max(axis=0) if len(finite) else np.zeros(3, np.float32)
        extent = [float(hi[a]) - float(lo[a]) for a in range(3)]
        dims, inv, edge = choose_grid(extent, len(finite), edge0)
        _GRIDS[(name, edge0)] = dict(points=len(p), finite_points=len(finite), lo=lo, hi=hi, dims=dims, inv=inv, cell_edge=edge,
                                     cells=dims[0] * dims[1] * dims[2])
    return _GRIDS[(name, edge0)]


# ---- the query sets -------------------------------------------------------------------------------------------------------------
QUERY_SETS = ("self", "around", "non_finite")
_QUERIES = {}


def queries(name, which):
    """self: the target cloud; around: 512 random points inside and around its box; non_finite: 64 points, most of them
    with a NaN or an infinity somewhere (shared: never changed by a test)"""
    if (name, which) not in _QUERIES:
        m = model(name)
        rng = np.random.RandomState(100 + NAMES.index(name))
        span = np.maximum(m["hi"].astype(np.float64) - m["lo"].astype(np.float64), 1.0)
        around = rng.uniform(m["lo"] - 0.6 * span, m["hi"] + 0.6 * span, (512, 3)).astype(np.float32)
        if which == "self":
            q = ZOO[name]
        elif which == "around":
            q = around
        else:
            q = around[:64].copy()
            q[0::4, 0] = np.nan
            q[1::4, 1] = np.inf
            q[2::8, 2] = -np.inf
            q[6] = [np.nan, np.nan, np.nan]
        q = np.ascontiguousarray(q, np.float32)
        q.setflags(write=False)
        _QUERIES[(name, which)] = q
    return _QUERIES[(name, which)]


# ---- the schedule (include/dliom.h, dliom_nn_index_create_batch) -----------------------------------------------------------------------
def chunks(sizes, max_indices, max_points):
    """-> [(first, end)]: consecutive clouds until the chunk holds max_indices, or the next cloud's points would take its sum
    above max_points; at least one cloud a chunk"""
    out, first = [], 0
    while first < len(sizes):
        end, points = first, 0
        while end < len(sizes) and end - first < max_indices:
            if end > first and points + sizes[end] > max_points:
                break
            points += sizes[end]
            end += 1
        out.append((first, end))
        first = end
    return out


def cell_runs(cells, max_cells):
    """the cell runs of ONE chunk whose indices have these cell counts -> [(first, end)]: consecutive indices whose
    cells + 1 sum to at most max_cells; at least one index a run"""
    out, first = [], 0
    while first < len(cells):
        end, entries = first, 0
        while end < len(cells):
            if end > first and entries + cells[end] + 1 > max_cells:
                break
            entries += cells[end] + 1
            end += 1
        out.append((first, end))
        first = end
    return out


def expected_stats(sizes, finite, cells, max_indices=DEFAULT_MAX_INDICES, max_points=DEFAULT_MAX_POINTS, max_cells=DEFAULT_MAX_CELLS):
    """the statistics of a call on clouds of these sizes whose indices have these finite counts and cell counts"""
    cut = chunks(sizes, max_indices, max_points)
    return dict(indices=len(sizes), chunks=len(cut), cell_runs=sum(len(cell_runs(cells[a:b], max_cells)) for a, b in cut),
                points=sum(sizes), finite_points=sum(finite), cells=sum(cells), read_backs=len(cut), synchronizations=len(cut),
                max_in_flight=max([b - a for a, b in cut], default=0))
