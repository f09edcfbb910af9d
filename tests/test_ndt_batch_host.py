"""Batched NDT without a GPU: the new names and struct layouts against the header, the limits, the scratch function, the
refusals that need no device, the Python statement of the schedule that tests/test_gpu_ndt_batch.py holds the device's
statistics against, and the zoo's properties under the CPU model (so that the GPU test's expectations are not vacuous)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_batch_common as bc  # noqa: E402
import ndt_common as nd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, A, H = nd.EVAL_GRADIENT, nd.EVAL_ALL, nd.EVAL_HESSIAN


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_symbols_and_constants(dl):
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    assert int(re.search(r"#define DLIOM_NDT_BATCH_MAX_PAIRS (\d+)", header).group(1)) == dl.NDT_BATCH_MAX_PAIRS == 256
    assert re.search(r"#define DLIOM_NDT_BATCH_DEFAULT_POINTS \(64 \* 1024\)", header) and dl.NDT_BATCH_DEFAULT_POINTS == 64 * 1024
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_ndt_batch_default_limits", "dliom_ndt_batch_scratch_bytes", "dliom_ndt_align_batch"):
        assert re.search(r"\b%s\(" % n, header), n  # declared
        assert n in names and getattr(dl.load_library(), n) is not None  # bound and exported
    for n in ("ndt_align_batch", "ndt_batch_default_limits", "ndt_batch_scratch_bytes"):
        assert callable(getattr(dl, n))


def test_struct_layouts_match_header(dl, tmp_path):
    fields = [("dliom_ndt_pair", dl.NdtPair), ("dliom_ndt_batch_limits", dl.NdtBatchLimits), ("dliom_ndt_batch_stats", dl.NdtBatchStats)]
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
    assert C.sizeof(dl.NdtPair) == 3 * 8 + 128 and C.sizeof(dl.NdtBatchLimits) == 16
    assert C.sizeof(dl.NdtBatchStats) == 8 * 8 + 3 * 8 + 8 + 4 * 8


def test_default_limits(dl):
    lim = dl.ndt_batch_default_limits()
    assert 1 <= lim.max_pairs_in_flight <= dl.NDT_BATCH_MAX_PAIRS and lim.reserved == 0 and lim.max_scratch_bytes > 0
    assert lim.max_pairs_in_flight == 64
    # the defaults hold a full chunk of the ground-truth tool's raw scans (64 x 1024 points), derived from the scratch function
    assert lim.max_pairs_in_flight * dl.ndt_batch_scratch_bytes(64 * 1024) <= lim.max_scratch_bytes
    assert lim.max_scratch_bytes == 64 * dl.ndt_batch_scratch_bytes(dl.NDT_BATCH_DEFAULT_POINTS) > 1 << 30
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    assert "{:,}".format(lim.max_scratch_bytes).replace(",", " ") + " bytes" in header  # the header states the number
    assert dl.ndt_batch_default_limits(max_pairs_in_flight=3).max_pairs_in_flight == 3
    with pytest.raises(TypeError):
        dl.ndt_batch_default_limits(no_such_limit=1)
    assert dl.load_library().dliom_ndt_batch_default_limits(None) == dl.ERR_INVALID_ARGUMENT


def test_scratch_bytes(dl):
    sizes = list(bc.SOURCE_SIZES) + [65536, 65537, 1 << 20]
    got = [dl.ndt_batch_scratch_bytes(n) for n in sizes]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[0] < got[-1]
    assert all(b % 256 == 0 for b in got)
    for n, b in zip(sizes, got):
        # the leaves alone are 28 doubles a point; the final round's arrays are the ICP batch's
        assert b >= 28 * 8 * n + 4 * n + 32 * n, n
        assert b <= 1024 + 256 + (28 * 8 + 4 + 32) * max(n, 1) + 12 * 256 + 3 * (28 + 16 + 1) * 8 * max(1, n // 1024), n
    assert dl.ndt_batch_scratch_bytes(-1) == 0


def test_refusals_without_a_device(dl):
    L = dl.load_library()
    o, lim = dl.ndt_options(), dl.ndt_batch_default_limits()
    results, stats, pairs = (dl.NdtResult * 1)(), dl.NdtBatchStats(), (dl.NdtPair * 1)()
    bad = dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_align_batch(None, None, 0, None, None, None, None, None) == bad
    assert L.dliom_ndt_align_batch(None, pairs, 1, C.byref(o), C.byref(lim), results, None, C.byref(stats)) == bad  # no context
    assert L.dliom_ndt_align_batch(None, pairs, -1, C.byref(o), C.byref(lim), results, None, C.byref(stats)) == bad
    assert L.dliom_ndt_align_batch(None, pairs, 0, C.byref(o), None, results, None, None) == bad  # count 0 still wants a context


def test_schedule_statement_by_hand():
    sizes = [100, 200, 300, 50]
    # one chunk, clamped: the max of the rounds, one kind, mixed only where a final round meets an evaluation
    seq = [[A, A, A], [A], [A, A, A, A, A], [A, A]]
    st = bc.expected_stats(seq, [True, True, False, False], [10, 10, 10, 10], sizes, 256, 1 << 40)
    assert st == dict(pairs=4, chunks=1, steps=5, read_backs=5, max_in_flight=4, pair_evaluations=11, pair_searches=2,
                      evaluation_launches=[0, 5, 0], mixed_steps=2)  # rounds 1 (pair 1's final) and 3 (pair 0's)
    # More-Thuente: round 2 runs all three kinds; pair 1 is empty and launches nothing of its own
    seq = [[A, A, G, G, H], [A, A, A], [A, A, H], [A]]
    st = bc.expected_stats(seq, [False, False, False, True], [10, 0, 10, 10], sizes, 256, 1 << 40)
    assert st == dict(pairs=4, chunks=1, steps=5, read_backs=5, max_in_flight=4, pair_evaluations=12, pair_searches=1,
                      evaluation_launches=[2, 2, 2], mixed_steps=2)  # round 1: A + final; round 2: G + H (the empty pair's A is no launch)
    # two pairs a chunk: the chunks' rounds add up
    st = bc.expected_stats(seq, [False, False, False, True], [10, 0, 10, 10], sizes, 2, 1 << 40)
    assert (st["chunks"], st["steps"], st["max_in_flight"]) == (2, 5 + 3, 2)
    assert st["evaluation_launches"] == [2, 2 + 2, 1 + 1] and st["mixed_steps"] == 1  # only chunk 2's round 1: A beside a final round
    # one pair a chunk: no sharing at all
    st = bc.expected_stats(seq, [False, False, False, True], [10, 0, 10, 10], sizes, 1, 1 << 40)
    assert st["steps"] == 12 + 1 and st["mixed_steps"] == 0 and st["evaluation_launches"] == [2, 5, 2]
    # by bytes
    assert bc.chunks(sizes, 256, 300) == [(0, 2), (2, 3), (3, 4)]
    assert bc.chunks(sizes, 256, 1) == [(i, i + 1) for i in range(4)]
    assert bc.expected_stats([], [], [], [], 4, 100) == dict(pairs=0, chunks=0, steps=0, read_backs=0, max_in_flight=0, pair_evaluations=0,
                                                             pair_searches=0, evaluation_launches=[0, 0, 0], mixed_steps=0)
    assert bc.rounds_of([A, A, G], True) == 4 and bc.rounds_of([A], False) == 1


def test_zoo_is_not_vacuous():
    """Under the CPU model with the More-Thuente search, the zoo has gradient-only and Hessian-only evaluations, pairs
    that leave a chunk at different rounds, and one pair for each way an alignment ends"""
    targets, pairs = bc.zoo_pairs()
    assert sorted({len(s) for _, s, _, _ in pairs}) == sorted(bc.SOURCE_SIZES) and {t for t, _, _, _ in pairs} == set(targets)
    o = nd.options(**bc.ZOO_OPTIONS)
    cells = {name: nd.build_cells(points, o) for name, points in targets.items()}
    assert cells["none"]["valid"].sum() == 0 and cells["one"]["valid"].sum() == 1 and 250 <= cells["scene"]["valid"].sum() <= 300
    assert 3000 <= len(targets["scene"]) <= 5000
    assert {f for _, _, _, f in pairs} == {True, False} and {g is None for _, _, g, _ in pairs} == {True, False}
    model = bc.zoo_model(nd.STEP_MORE_THUENTE)
    kinds = [k for _, k in model]
    assert any(G in k for k in kinds) and any(H in k for k in kinds) and all(k[0] == A for k in kinds)
    assert len({len(k) for k in kinds}) > 2  # a chunk does shrink
    reasons = {r["reason"] for r, _ in model}
    assert reasons == {nd.ZERO_STEP, nd.ITERATIONS, nd.EPSILON}
    assert all(r["iterations"] == bc.ZOO_OPTIONS["maximum_iterations"] + 2 for r, _ in model if r["reason"] == nd.ITERATIONS)
    for r, k in model:
        assert r["evaluations_with_hessian"] == sum(1 for w in k if w != G) and r["evaluations_without_hessian"] == k.count(G)
    clamped = bc.zoo_model(nd.STEP_CLAMPED)
    assert all(set(k) == {A} for _, k in clamped) and len({len(k) for _, k in clamped}) > 2
    # the first 2, 3 and 17 pairs under More-Thuente launch every kind and mix rounds (what the GPU test asserts of the device)
    sizes = [len(s) for _, s, _, _ in pairs]
    st = bc.expected_stats(kinds, [True] * 17, sizes, [1] * 17, 256, 1 << 40)
    assert st["mixed_steps"] > 0 and all(v > 0 for v in st["evaluation_launches"])
