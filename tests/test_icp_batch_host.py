"""Batched ICP without a GPU: the new names and struct layouts against the header, the limits, the scratch function, the
refusals that need no device, and the Python statement of the schedule that tests/test_gpu_icp_batch.py holds the
device's statistics against."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_batch_common as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_symbols_and_constants(dl):
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    assert int(re.search(r"#define DLIOM_ICP_BATCH_MAX_PAIRS (\d+)", header).group(1)) == dl.ICP_BATCH_MAX_PAIRS == 256
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_icp_batch_default_limits", "dliom_icp_batch_scratch_bytes", "dliom_icp_align_batch"):
        assert n in names and getattr(dl.load_library(), n) is not None
    for n in ("icp_align_batch", "icp_batch_default_limits", "icp_batch_scratch_bytes"):
        assert callable(getattr(dl, n))


def test_struct_layouts_match_header(dl, tmp_path):
    fields = [("dliom_icp_pair", dl.IcpPair), ("dliom_icp_batch_limits", dl.IcpBatchLimits), ("dliom_icp_batch_stats", dl.IcpBatchStats)]
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
    assert C.sizeof(dl.IcpPair) == 8 + 8 + 128 and C.sizeof(dl.IcpBatchLimits) == 16 and C.sizeof(dl.IcpBatchStats) == 7 * 8 + 4 * 8


def test_default_limits(dl):
    lim = dl.icp_batch_default_limits()
    assert 1 <= lim.max_pairs_in_flight <= dl.ICP_BATCH_MAX_PAIRS and lim.reserved == 0 and lim.max_scratch_bytes > 0
    assert (lim.max_pairs_in_flight, lim.max_scratch_bytes) == (64, 1 << 30)
    # the defaults hold a full chunk of the ground-truth tool's raw scans (64 x 1024 points)
    assert lim.max_pairs_in_flight * dl.icp_batch_scratch_bytes(64 * 1024) <= lim.max_scratch_bytes
    assert dl.icp_batch_default_limits(max_pairs_in_flight=3).max_pairs_in_flight == 3
    with pytest.raises(TypeError):
        dl.icp_batch_default_limits(no_such_limit=1)
    assert dl.load_library().dliom_icp_batch_default_limits(None) == dl.ERR_INVALID_ARGUMENT


def test_scratch_bytes_positive_and_monotone(dl):
    sizes = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 65536, 65537, 1 << 20, 1 << 24]
    got = [dl.icp_batch_scratch_bytes(n) for n in sizes]
    assert got[0] > 0
    assert all(a <= b for a, b in zip(got, got[1:])) and got[0] < got[-1]
    assert all(b % 256 == 0 for b in got)
    # a point costs at least its three coordinates, its neighbour, its distance, its list entry and its 64-bit key
    assert got[sizes.index(65536)] >= 65536 * 32
    assert dl.icp_batch_scratch_bytes(-1) == 0


def test_refusals_without_a_device(dl):
    L = dl.load_library()
    o, lim = dl.icp_options(), dl.icp_batch_default_limits()
    results, stats, pairs = (dl.IcpResult * 1)(), dl.IcpBatchStats(), (dl.IcpPair * 1)()
    bad = dl.ERR_INVALID_ARGUMENT
    assert L.dliom_icp_align_batch(None, None, 0, None, None, None, None, None) == bad
    assert L.dliom_icp_align_batch(None, pairs, 1, C.byref(o), C.byref(lim), results, None, C.byref(stats)) == bad  # no context
    assert L.dliom_icp_align_batch(None, pairs, -1, C.byref(o), C.byref(lim), results, None, C.byref(stats)) == bad
    assert L.dliom_icp_align_batch(None, pairs, 0, C.byref(o), None, results, None, None) == bad  # count 0 still wants a context


@pytest.mark.parametrize("max_pairs", [1, 2, 3, 16, 256])
def test_schedule_by_pairs(max_pairs):
    sizes = [100] * 7
    runs = bc.chunks(sizes, max_pairs, 1 << 40)
    assert runs[0][0] == 0 and runs[-1][1] == 7 and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert all(b - a == max_pairs for a, b in runs[:-1]) and 1 <= runs[-1][1] - runs[-1][0] <= max_pairs
    assert len(runs) == -(-7 // max_pairs)


def test_schedule_by_bytes_and_steps():
    sizes = [100, 200, 300, 50, 1000, 10]
    assert bc.chunks(sizes, 256, 1 << 40) == [(0, 6)]
    assert bc.chunks(sizes, 256, 300) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]  # 1000 alone exceeds 300: a chunk of its own
    assert bc.chunks(sizes, 256, 650) == [(0, 4), (4, 5), (5, 6)]  # 100 + 200 + 300 + 50 == 650 fits exactly
    assert bc.chunks(sizes, 256, 649) == [(0, 3), (3, 4), (4, 5), (5, 6)]  # 50 + 1000 > 649, and 1000 + 10 > 649
    assert bc.chunks(sizes, 256, 1010) == [(0, 4), (4, 6)]
    assert bc.chunks(sizes, 2, 649) == [(0, 2), (2, 4), (4, 5), (5, 6)]
    assert bc.chunks(sizes, 256, 1) == [(i, i + 1) for i in range(6)]  # smaller than any pair's need: one pair a chunk
    assert bc.chunks([], 4, 100) == []
    searches = [5, 2, 7, 2, 3, 9]
    st = bc.expected_stats(searches, sizes, 256, 1 << 40)
    assert st == dict(pairs=6, chunks=1, steps=9, read_backs=9, pair_searches=28, max_in_flight=6)  # the max, not the sum
    st = bc.expected_stats(searches, sizes, 2, 1 << 40)
    assert st == dict(pairs=6, chunks=3, steps=5 + 7 + 9, read_backs=21, pair_searches=28, max_in_flight=2)
    st = bc.expected_stats(searches, sizes, 1, 1 << 40)
    assert st["steps"] == st["pair_searches"] == 28 and st["chunks"] == 6
    assert bc.expected_stats([], [], 4, 100) == dict(pairs=0, chunks=0, steps=0, read_backs=0, pair_searches=0, max_in_flight=0)
