"""The batched NDT target build without a GPU: the new names and struct layouts against the header, the limits, the
refusals that need no device, the Python statement of the schedule that tests/test_gpu_ndt_target_batch.py holds the
device's statistics against, and the zoo's properties under the CPU model (so that the GPU test's cases are not vacuous)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_target_batch_common as tb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_symbols_and_constants(dl):
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    assert int(re.search(r"#define DLIOM_NDT_TARGET_BATCH_MAX_TARGETS (\d+)", header).group(1)) == dl.NDT_TARGET_BATCH_MAX_TARGETS == 256
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_ndt_target_batch_default_limits", "dliom_ndt_target_create_batch"):
        assert re.search(r"\b%s\(" % n, header), n  # declared
        assert n in names and getattr(dl.load_library(), n) is not None  # bound and exported
    for n in ("ndt_targets_batch", "ndt_target_batch_default_limits"):
        assert callable(getattr(dl, n))
    # the first read-back, two words a target, fits the small read-backs' region of the page-locked block
    layout = open(os.path.join(ROOT, "d-liom_amd", "csrc", "pinned_layout.h")).read()
    readback = int(re.search(r"constexpr PinRegion kPinReadback\{0, (\d+)\}", layout).group(1))
    assert 2 * 4 * dl.NDT_TARGET_BATCH_MAX_TARGETS <= readback


def test_struct_layouts_match_header(dl, tmp_path):
    fields = [("dliom_ndt_target_batch_limits", dl.NdtTargetBatchLimits), ("dliom_ndt_target_batch_stats", dl.NdtTargetBatchStats)]
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
    assert C.sizeof(dl.NdtTargetBatchLimits) == 16 and C.sizeof(dl.NdtTargetBatchStats) == 10 * 8 + 4 * 8


def test_default_limits(dl):
    lim = dl.ndt_target_batch_default_limits()
    assert (lim.max_targets_in_flight, lim.reserved, lim.max_points_in_flight) == (64, 0, 64 * dl.NDT_BATCH_DEFAULT_POINTS)
    assert (lim.max_targets_in_flight, lim.max_points_in_flight) == (tb.DEFAULT_MAX_TARGETS, tb.DEFAULT_MAX_POINTS)
    assert dl.ndt_target_batch_default_limits(max_targets_in_flight=3).max_targets_in_flight == 3
    with pytest.raises(TypeError):
        dl.ndt_target_batch_default_limits(no_such_limit=1)
    assert dl.load_library().dliom_ndt_target_batch_default_limits(None) == dl.ERR_INVALID_ARGUMENT


def test_refusals_without_a_device(dl):
    L = dl.load_library()
    o, lim, stats = dl.ndt_options(), dl.ndt_target_batch_default_limits(), dl.NdtTargetBatchStats()
    bad = dl.ERR_INVALID_ARGUMENT
    sentinel = 0x5a5a

    def call(ctx, clouds, count, options, limits, with_out=True):
        out = (C.c_void_p * 2)(sentinel, sentinel)
        status = L.dliom_ndt_target_create_batch(ctx, clouds, count, None if options is None else C.byref(options),
                                                 None if limits is None else C.byref(limits), out if with_out else None, C.byref(stats))
        return status, [out[0], out[1]]

    clouds = (C.c_void_p * 2)()
    assert call(None, None, 0, None, None, with_out=False)[0] == bad
    assert call(None, clouds, 2, o, lim) == (bad, [None, None])  # no context; every out[i] is NULL
    assert call(None, clouds, 0, o, None) == (bad, [sentinel, sentinel])  # count 0 still wants a context
    assert call(None, clouds, -1, o, lim) == (bad, [sentinel, sentinel])
    assert call(None, clouds, 2, o, lim, with_out=False)[0] == bad


def test_schedule_statement_by_hand():
    sizes = [100, 200, 300, 50]
    assert tb.chunks(sizes, 256, 1 << 30) == [(0, 4)]
    assert tb.chunks(sizes, 3, 1 << 30) == [(0, 3), (3, 4)]
    assert tb.chunks(sizes, 1, 1 << 30) == [(i, i + 1) for i in range(4)]
    assert tb.chunks(sizes, 256, 300) == [(0, 2), (2, 3), (3, 4)]  # 100 + 200 fits exactly; 300 alone; 50 alone after it
    assert tb.chunks(sizes, 256, 299) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert tb.chunks(sizes, 256, 1) == [(i, i + 1) for i in range(4)]  # a chunk always holds one cloud
    assert tb.chunks(sizes, 256, 350) == [(0, 2), (2, 4)]
    assert tb.chunks([], 4, 100) == []
    kept, cells, valid = [90, 0, 300, 0], [7, 0, 20, 0], [3, 0, 11, 0]
    # one chunk: two read-backs, since some target has a cell
    assert tb.expected_stats(sizes, kept, cells, valid, 256, 1 << 30) == dict(
        targets=4, chunks=1, points=650, kept_points=390, cells=27, valid_cells=14, read_backs=2, synchronizations=1, max_in_flight=4)
    # a cloud a chunk: the two clouds without a cell cost one read-back each
    st = tb.expected_stats(sizes, kept, cells, valid, 1, 1 << 30)
    assert (st["chunks"], st["read_backs"], st["synchronizations"], st["max_in_flight"]) == (4, 2 + 1 + 2 + 1, 4, 1)
    assert tb.target_read_backs(sizes, cells, 1, 1 << 30) == [2, 1, 2, 1]
    assert tb.target_read_backs(sizes, cells, 256, 300) == [2, 2, 2, 1]
    assert tb.expected_stats([], [], [], []) == dict(targets=0, chunks=0, points=0, kept_points=0, cells=0, valid_cells=0,
                                                     read_backs=0, synchronizations=0, max_in_flight=0)


def test_zoo_is_not_vacuous():
    assert len(tb.NAMES) == 11 and tb.first_k(17)[11:] == tb.NAMES[:6]
    assert [len(tb.ZOO["n%d" % n]) for n in (1, 255, 256, 257, 2049)] == [1, 255, 256, 257, 2049]
    lengths = tb.model("lengths")
    assert lengths["n"].max() > 4000 and ((lengths["n"] > 256) & (lengths["n"] < 600)).any()  # cells crossing the 256-leaf chunk
    assert lengths["n"].min() < 6 and lengths["valid"].sum() >= 5
    # an invalid cell of each kind: too few points; enough points and a covariance that the statement refuses
    degenerate = tb.model("degenerate")
    assert ((degenerate["n"] < 6) & ~degenerate["valid"]).any() and ((degenerate["n"] >= 6) & ~degenerate["valid"]).any()
    assert degenerate["valid"].any() and degenerate["kept_points"] < len(tb.ZOO["degenerate"])  # its sorted run ends on skip keys
    # equal keys at a target boundary: `one` is a single cell, so one|one meets on its key; degenerate|none on the skip key
    one, none = tb.model("one"), tb.model("none")
    assert len(one["n"]) == 1 and one["valid"].all()
    assert len(none["n"]) == 0 and none["kept_points"] == 0 and len(tb.ZOO["none"]) == 5
    assert len(tb.model("sparse")["n"]) < 200 and tb.model("sparse")["valid"].sum() >= 8
    # clouds whose ends are neither a workgroup's nor a cell's, with skipped points inside
    for n in (255, 256, 257, 2049):
        m = tb.model("n%d" % n)
        assert m["kept_points"] == n - 2 and len(m["n"]) > 8
    assert tb.model("n1")["n"].tolist() == [1]
