"""What tests/test_gpu_ndt_target_batch.py and tests/test_ndt_target_batch_host.py share: the zoo of target clouds, their
cells under the CPU model (tests/ndt_common.py, computed once a process), and the Python statement of
dliom_ndt_target_create_batch's schedule that the device's statistics are held against."""
import numpy as np

import ndt_common as nd

DEFAULT_MAX_TARGETS, DEFAULT_MAX_POINTS = 64, 64 * 64 * 1024


def blob(rng, centre, n, spread=0.15):
    return (np.asarray(centre) + spread * rng.standard_normal((n, 3))).astype(np.float32)


def cloud_of_size(n, seed):
    """n points over a 4 x 4 x 2 box of cells and a few skipped ones, so that a cloud's end is neither a cell's nor a
    workgroup's"""
    rng = np.random.RandomState(seed)
    p = rng.uniform([0.0, 0.0, 0.0], [4.0, 4.0, 2.0], (n, 3)).astype(np.float32)
    if n >= 16:
        p[n // 2] = [np.nan, 0.5, 0.5]
        p[n // 3] = [0.5, 3e6, 0.5]
    return p


def _zoo():
    z = {}
    rng = np.random.RandomState(1)  # tests/test_gpu_ndt.py::test_cells_of_every_length
    sizes = [1, 2, 3, 5, 6, 255, 256, 257, 4097]
    points = np.concatenate([blob(rng, [2.0 * k + 0.5, 0.5, 0.5], n, 0.1) for k, n in enumerate(sizes)])
    z["lengths"] = points[rng.permutation(len(points))]
    rng = np.random.RandomState(2)  # ::test_cells_on_faces_negative_and_rounding
    faces = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0], np.float32)
    near = np.concatenate([faces, np.nextafter(faces, np.float32(-9)), np.nextafter(faces, np.float32(9))])
    grid = np.stack(np.meshgrid(near, near[:6], [0.25, -0.25]), axis=-1).reshape(-1, 3).astype(np.float32)
    z["faces"] = np.concatenate([grid, blob(rng, [-3.5, -2.5, -1.5], 40), blob(rng, [-0.5, 0.5, -0.5], 40)])
    rng = np.random.RandomState(3)  # ::test_degenerate_cells
    flat = np.c_[rng.uniform(0.1, 0.9, (20, 2)), np.full(20, 0.5)].astype(np.float32)
    same = np.tile(np.array([[1.5, 0.5, 0.5]], np.float32), (9, 1))
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [3e6, 0.5, 0.5], [0.5, -1.2e6, 0.5]], np.float32)
    edge = np.array([[1048575.5, 0.5, 0.5], [-1048576.0, 0.5, 0.5]], np.float32)
    z["degenerate"] = np.concatenate([flat, bad, same, edge, blob(rng, [4.5, 0.5, 0.5], 30)])
    rng = np.random.RandomState(4)  # ::test_sparse_box
    a = np.concatenate([blob(rng, [0.5 + k, 0.5, 0.5], 12) for k in range(6)])
    z["sparse"] = np.concatenate([a, a + np.array([3000.0, -3000.0, 3000.0], np.float32)])
    for k, n in enumerate((1, 255, 256, 257, 2049)):
        z["n%d" % n] = cloud_of_size(n, 10 + k)
    z["none"] = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2.2e6, 0.5, 0.5], [0.5, 0.5, -3e6], [np.nan, np.nan, np.nan]], np.float32)
    rng = np.random.RandomState(6)
    z["one"] = (np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (16, 3))).astype(np.float32)
    for v in z.values():
        v.setflags(write=False)
    return z


ZOO = _zoo()
NAMES = list(ZOO)  # 11 clouds
_CELLS = {}


def model(name, **overrides):
    """the model's cells of a zoo cloud (shared: never changed by a test)"""
    key = (name, tuple(sorted(overrides.items())))
    if key not in _CELLS:
        _CELLS[key] = nd.build_cells(ZOO[name], nd.options(**overrides))
    return _CELLS[key]


def first_k(k):
    """the first k names of the zoo, going round it again beyond its end"""
    return [NAMES[i % len(NAMES)] for i in range(k)]


# ---- the schedule (include/dliom.h, dliom_ndt_target_create_batch) -----------------------------------------------------------------
def chunks(sizes, max_targets, max_points):
    """-> [(first, end)]: consecutive clouds until the chunk holds max_targets, or the next cloud's points would take its sum
    above max_points; at least one cloud a chunk"""
    out, first = [], 0
    while first < len(sizes):
        end, points = first, 0
        while end < len(sizes) and end - first < max_targets:
            if end > first and points + sizes[end] > max_points:
                break
            points += sizes[end]
            end += 1
        out.append((first, end))
        first = end
    return out


def expected_stats(sizes, kept, cells, valid, max_targets=DEFAULT_MAX_TARGETS, max_points=DEFAULT_MAX_POINTS):
    """the statistics of a call on clouds of these sizes whose targets have these kept, cell and valid-cell counts"""
    cut = chunks(sizes, max_targets, max_points)
    return dict(targets=len(sizes), chunks=len(cut), points=sum(sizes), kept_points=sum(kept), cells=sum(cells),
                valid_cells=sum(valid), read_backs=sum(2 if sum(cells[a:b]) > 0 else 1 for a, b in cut),
                synchronizations=len(cut), max_in_flight=max([b - a for a, b in cut], default=0))


def target_read_backs(sizes, cells, max_targets=DEFAULT_MAX_TARGETS, max_points=DEFAULT_MAX_POINTS):
    """every target's read_backs: its chunk's"""
    out = []
    for a, b in chunks(sizes, max_targets, max_points):
        out += [2 if sum(cells[a:b]) > 0 else 1] * (b - a)
    return out
