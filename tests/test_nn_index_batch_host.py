"""The batched index build without a GPU: the new names and struct layouts against the header, the limits, the refusals
that need no device, the Python statement of the schedule that tests/test_gpu_nn_index_batch.py holds the device's
statistics against, and the zoo's properties under the grid's model (so that the GPU test's cases are not vacuous)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_index_batch_common as nb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_symbols_and_constants(dl):
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    assert int(re.search(r"#define DLIOM_NN_INDEX_BATCH_MAX_INDICES (\d+)", header).group(1)) == dl.NN_INDEX_BATCH_MAX_INDICES == 256
    assert (nb.MAX_CELLS_PER_AXIS, nb.MAX_CELLS) == (dl.NN_MAX_CELLS_PER_AXIS, dl.NN_MAX_CELLS)
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_nn_index_batch_default_limits", "dliom_nn_index_create_batch"):
        assert re.search(r"\b%s\(" % n, header), n  # declared
        assert n in names and getattr(dl.load_library(), n) is not None  # bound and exported
    for n in ("nn_indices_batch", "nn_index_batch_default_limits"):
        assert callable(getattr(dl, n))
    assert callable(dl.NnIndex._adopt)
    # the boxes' read-back, eight words a cloud, has a region of its own: it would not fit the small read-backs'
    layout = open(os.path.join(ROOT, "d-liom_amd", "csrc", "pinned_layout.h")).read()
    readback = int(re.search(r"constexpr PinRegion kPinReadback\{0, (\d+)\}", layout).group(1))
    assert 8 * 4 * dl.NN_INDEX_BATCH_MAX_INDICES > readback
    assert "kPinNnIndexBatchTable" in layout and "kPinNnIndexBatchBoxes" in layout


def test_struct_layouts_match_header(dl, tmp_path):
    fields = [("dliom_nn_index_batch_limits", dl.NnIndexBatchLimits), ("dliom_nn_index_batch_stats", dl.NnIndexBatchStats)]
    exprs, want = [], []
    for name, t in fields:
        exprs.append("sizeof(%s)" % name)
        want.append(C.sizeof(t))
        for f, _ in t._fields_:
            exprs.append("offsetof(%s, %s)" % (name, f))
            want.append(getattr(t, f).offset)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dliom.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * len(exprs)), ", ".join(exprs)))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == want
    assert C.sizeof(dl.NnIndexBatchLimits) == 24 and C.sizeof(dl.NnIndexBatchStats) == 10 * 8 + 3 * 8


def test_default_limits(dl):
    lim = dl.nn_index_batch_default_limits()
    assert (lim.max_indices_in_flight, lim.reserved, lim.max_points_in_flight, lim.max_cells_in_flight) == \
        (64, 0, 64 * dl.NDT_BATCH_DEFAULT_POINTS, 1 << 26)
    assert (lim.max_indices_in_flight, lim.max_points_in_flight, lim.max_cells_in_flight) == \
        (nb.DEFAULT_MAX_INDICES, nb.DEFAULT_MAX_POINTS, nb.DEFAULT_MAX_CELLS)
    assert dl.nn_index_batch_default_limits(max_cells_in_flight=3).max_cells_in_flight == 3
    with pytest.raises(TypeError):
        dl.nn_index_batch_default_limits(no_such_limit=1)
    assert dl.load_library().dliom_nn_index_batch_default_limits(None) == dl.ERR_INVALID_ARGUMENT


def test_refusals_without_a_device(dl):
    L = dl.load_library()
    o, lim, stats = dl.NnIndexOptions(0.0, dl.NN_AUTO, 0), dl.nn_index_batch_default_limits(), dl.NnIndexBatchStats()
    bad = dl.ERR_INVALID_ARGUMENT
    sentinel = 0x5a5a

    def call(ctx, clouds, count, options, limits, with_out=True):
        out = (C.c_void_p * 2)(sentinel, sentinel)
        status = L.dliom_nn_index_create_batch(ctx, clouds, count, None if options is None else C.byref(options),
                                               None if limits is None else C.byref(limits), out if with_out else None, C.byref(stats))
        return status, [out[0], out[1]]

    clouds = (C.c_void_p * 2)()
    assert call(None, None, 0, None, None, with_out=False)[0] == bad
    assert call(None, clouds, 2, o, lim) == (bad, [None, None])  # no context; every out[i] is NULL
    assert call(None, clouds, 0, None, None) == (bad, [sentinel, sentinel])  # count 0 still wants a context
    assert call(None, clouds, -1, o, lim) == (bad, [sentinel, sentinel])
    assert call(None, clouds, 2, o, lim, with_out=False)[0] == bad


def test_schedule_statement_by_hand():
    sizes = [100, 200, 300, 50]
    assert nb.chunks(sizes, 256, 1 << 30) == [(0, 4)]
    assert nb.chunks(sizes, 3, 1 << 30) == [(0, 3), (3, 4)]
    assert nb.chunks(sizes, 1, 1 << 30) == [(i, i + 1) for i in range(4)]
    assert nb.chunks(sizes, 256, 300) == [(0, 2), (2, 3), (3, 4)]  # 100 + 200 fits exactly; 300 alone; 50 alone after it
    assert nb.chunks(sizes, 256, 299) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert nb.chunks(sizes, 256, 1) == [(i, i + 1) for i in range(4)]  # a chunk always holds one cloud
    assert nb.chunks([], 4, 100) == []
    cells = [9, 1, 30, 4]  # entries: 10, 2, 31, 5
    assert nb.cell_runs(cells, 1 << 30) == [(0, 4)]
    assert nb.cell_runs(cells, 48) == [(0, 4)]  # 10 + 2 + 31 + 5 fits exactly
    assert nb.cell_runs(cells, 47) == [(0, 3), (3, 4)]
    assert nb.cell_runs(cells, 12) == [(0, 2), (2, 3), (3, 4)]  # an index larger than the limit runs alone
    assert nb.cell_runs(cells, 1) == [(i, i + 1) for i in range(4)]
    assert nb.cell_runs([], 5) == []
    finite = [90, 0, 300, 50]
    assert nb.expected_stats(sizes, finite, cells, 256, 1 << 30, 1 << 30) == dict(
        indices=4, chunks=1, cell_runs=1, points=650, finite_points=440, cells=44, read_backs=1, synchronizations=1, max_in_flight=4)
    # the cell runs never cross a chunk: chunks (0, 2), (2, 3), (3, 4); the first one's entries 10 + 2 split at 11
    st = nb.expected_stats(sizes, finite, cells, 256, 300, 11)
    assert (st["chunks"], st["cell_runs"], st["read_backs"], st["synchronizations"], st["max_in_flight"]) == (3, 4, 3, 3, 2)
    assert nb.expected_stats([], [], []) == dict(indices=0, chunks=0, cell_runs=0, points=0, finite_points=0, cells=0, read_backs=0,
                                                 synchronizations=0, max_in_flight=0)


def test_grid_model_by_hand():
    # no extent, or an extent that is not finite: one cell with inv = 0
    assert nb.choose_grid([0.0, 0.0, 0.0], 2, 0.0) == ([1, 1, 1], 0.0, 0.0)
    assert nb.choose_grid([float("inf"), 1.0, 1.0], 5, 0.0)[0] == [1, 1, 1]
    # 1000 points in a 10 m cube: half the edge of a point's share of the volume, 0.5 m -> 21 cells an axis
    dims, inv, edge = nb.choose_grid([10.0, 10.0, 10.0], 1000, 0.0)
    assert dims == [21, 21, 21] and inv == np.float32(2.0) and edge == 0.5
    # a plane: the share of the area; a given edge is taken as it is when it fits
    assert nb.choose_grid([10.0, 10.0, 0.0], 100, 0.0)[0] == [21, 21, 1]
    assert nb.choose_grid([10.0, 10.0, 0.0], 100, 2.5)[0] == [5, 5, 1]
    # an edge that does not fit grows by 1.26 a step until it does
    dims, inv, edge = nb.choose_grid([1.0, 1.0, 1.0], 8, 1e-6)
    assert dims[0] * dims[1] * dims[2] <= nb.MAX_CELLS < 2.1 * dims[0] * dims[1] * dims[2] and max(dims) <= nb.MAX_CELLS_PER_AXIS
    steps = round(np.log(edge / 1e-6) / np.log(1.26))
    assert steps > 30 and abs(edge - 1e-6 * 1.26 ** steps) < 1e-6 * edge


def test_zoo_is_not_vacuous():
    assert len(nb.NAMES) == 14 and nb.first_k(17)[14:] == nb.NAMES[:3]
    m = {n: nb.model(n) for n in nb.NAMES}
    # a one-cell grid with inv = 0: one point, and two identical ones
    for n in ("p1", "same2"):
        assert (m[n]["dims"], float(m[n]["inv"]), m[n]["cell_edge"], m[n]["finite_points"]) == ([1, 1, 1], 0.0, 0.0, len(nb.ZOO[n]))
    assert np.array_equal(nb.ZOO["same2"][0], nb.ZOO["same2"][1])
    # a cloud without a finite point
    assert m["none"]["finite_points"] == 0 and m["none"]["points"] == 4 and m["none"]["cells"] == 1
    # one and two axes with an extent
    assert m["line"]["dims"][1:] == [1, 1] and m["line"]["dims"][0] > 100
    assert m["plane"]["dims"][2] == 1 and min(m["plane"]["dims"][:2]) > 10
    # lengths either side of a workgroup's 256 points and of 2048
    assert [m["n%d" % n]["points"] for n in (255, 256, 257, 2049)] == [255, 256, 257, 2049]
    assert all(m["n%d" % n]["finite_points"] == n - 2 and m["n%d" % n]["cells"] > 256 for n in (255, 256, 257, 2049))
    # finite and non-finite points mixed
    assert 0 < m["mixed"]["finite_points"] < m["mixed"]["points"] - 20
    assert np.isnan(nb.ZOO["mixed"]).any() and np.isposinf(nb.ZOO["mixed"]).any() and np.isneginf(nb.ZOO["mixed"]).any()
    # duplicated points on a lattice
    lattice = nb.ZOO["lattice"]
    assert len(np.unique(lattice, axis=0)) == 60 < len(lattice) == 110 and (lattice == np.round(lattice)).all()
    # two clusters 10 km apart: the automatic edge does not fit and is grown
    far = m["far"]
    extent = far["hi"].astype(np.float64) - far["lo"].astype(np.float64)
    first = 0.5 * (extent.prod() / far["finite_points"]) ** (1.0 / 3.0)
    assert extent[0] > 10000.0 and extent[0] / first > nb.MAX_CELLS_PER_AXIS and far["cell_edge"] > 1.26 * first
    assert far["dims"][0] <= nb.MAX_CELLS_PER_AXIS
    # the neighbours: equal length, equal box, hence equal grids, and different points
    a, b = m["twin_a"], m["twin_b"]
    assert nb.NAMES.index("twin_b") == nb.NAMES.index("twin_a") + 1
    assert a["points"] == b["points"] == 200 and np.array_equal(a["lo"], b["lo"]) and np.array_equal(a["hi"], b["hi"]) and a["dims"] == b["dims"]
    assert not np.array_equal(nb.ZOO["twin_a"], nb.ZOO["twin_b"])
    # the given edges: 1e-6 is grown to the cell cap wherever there is an extent
    for n in ("n257", "twin_a", "lattice"):
        grown = nb.model(n, 1e-6)
        assert nb.MAX_CELLS // 2 < grown["cells"] <= nb.MAX_CELLS and grown["cells"] > 1000 * grown["points"]
    assert nb.model("same2", 1e-6)["cells"] == 1 and nb.model("n257", 0.37)["cell_edge"] == 1.0 / float(np.float32(1.0 / 0.37))
    # the query sets
    for n in nb.NAMES:
        assert nb.queries(n, "self") is nb.ZOO[n] or np.array_equal(nb.queries(n, "self"), nb.ZOO[n], equal_nan=True)
        assert nb.queries(n, "around").shape == (512, 3) and np.isfinite(nb.queries(n, "around")).all()
        bad = nb.queries(n, "non_finite")
        assert bad.shape == (64, 3) and 30 < (~np.isfinite(bad).all(axis=1)).sum() < 64
