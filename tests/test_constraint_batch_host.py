"""Batched loop-closure calls (dliom_fast_csm_match_batch, dliom_csm3d_match_batch) without a GPU: the argument
checks refuse malformed input before anything runs, and the new names are bound."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_batch_symbols_exported(dl):
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_fast_csm_match_batch", "dliom_csm3d_match_batch", "dliom_ctx_synchronizations"):
        assert n in names
        assert getattr(dl.load_library(), n) is not None


def test_fast_csm_batch_argument_checks(dl):
    L = dl.load_library()
    q = (dl.FastCsmQuery * 1)()
    res = (dl.FastCsmResult * 1)()
    st = (C.c_int * 1)()
    stats = dl.BatchStats()
    assert L.dliom_fast_csm_match_batch(None, q, 1, res, st, C.byref(stats)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_fast_csm_match_batch(None, None, 0, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_fast_csm_match_batch(None, None, -1, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ctx_synchronizations(None, None) == dl.ERR_INVALID_ARGUMENT


def test_csm_batch_argument_checks(dl):
    L = dl.load_library()
    o = dl.CsmOptions()
    p = (dl.CsmProblem * 1)()
    poses = (C.c_double * 7)()
    st = (C.c_int * 1)()
    assert L.dliom_csm3d_match_batch(None, C.byref(o), 1, p, poses, None, st, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_csm3d_match_batch(None, None, 0, None, None, None, None, None) == dl.ERR_INVALID_ARGUMENT


def test_batch_struct_layouts_match_header(dl, tmp_path):
    """The ctypes mirrors of the three new structs have the header's sizes (a C program prints them)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "dliom.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(dliom_batch_stats), sizeof(dliom_fast_csm_query), sizeof(dliom_csm_problem)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(dl.BatchStats), C.sizeof(dl.FastCsmQuery), C.sizeof(dl.CsmProblem)]


def test_constraint_batch_adapter_compiles(dl, tmp_path):
    """tests/cpp/constraint_batch_adapter.cc (the adapter's MatchBatch / ComputeConstraints) builds with plain g++."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "d-liom_amd")
    exe = str(tmp_path / "constraint_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(root, "tests", "cpp", "constraint_batch_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
