"""The XYZ writer's text without a GPU: dliom_float_text (csrc/float_text.h on the host) against the CPU model -- the
reference's std::ostringstream loop -- and against Python's '%.6g', the stand-alone check program built plain and under
AddressSanitizer + UBSan, and the declarations, bindings and refusals of the new entry points."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xyz_text_common as xt  # noqa: E402

GROUPS = {"special": xt.special_values, "exponent_fields": xt.exponent_field_values, "decades": xt.decade_values,
          "ties": xt.tie_values}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return xt.build_model(tmp_path_factory.mktemp("xyz_writer_model"))


def test_named_ties_spelled_out(model, tmp_path):
    """The reference itself, pinned: correct rounding of the exact value with ties to even, not half away from zero."""
    values = np.array([v for v, _ in xt.NAMED_TEXTS], dtype=xt.f32)
    want = [t for _, t in xt.NAMED_TEXTS]
    assert xt.model_texts(model, values, tmp_path) == want
    assert [xt.python_text(v) for v in values] == want
    assert xt.run_model(model, np.array([[1000.125, -0.0, 1e-5]], dtype=xt.f32), tmp_path) == b"1000.12 -0 1e-05\n"


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_float_text_equals_model_and_python(model, tmp_path, group):
    import dliom
    values = GROUPS[group]()
    assert len(values) > 0
    want = xt.model_texts(model, values, tmp_path)
    for v, w in zip(values, want):
        got = dliom.float_text(v)
        assert got == w, (group, hex(int(v.view(np.uint32))), got, w)
        assert got == xt.python_text(v), (group, hex(int(v.view(np.uint32))), got)
        assert len(got) <= 12


def test_groups_hold_what_they_should():
    ties = xt.tie_values()
    for v in xt.NAMED_TIES:
        assert xt.f32(v) in ties and xt.f32(-v) in ties
    assert len(xt.exponent_field_values()) == 256 * 2 * 70
    decades = xt.decade_values()
    assert xt.f32(1e-45) in decades and xt.f32(1e38) in decades and xt.f32(999999.5) in decades
    pts = xt.stride_points(1 << 10)
    assert pts.shape == (1 << 10, 3) and pts.view(np.uint32)[0, 1] - pts.view(np.uint32)[0, 0] == 1367
    assert 3 * (1 << 20) * 1367 >= 1 << 32  # the sweep of the GPU test runs through all bit patterns


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_float_text_check_program(tmp_path, sanitize):
    """float_text.h compiled with its width assertions on, against snprintf on every 4099th bit pattern."""
    exe = xt.build_check(tmp_path, sanitize)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    text = done.stdout.decode()
    assert done.returncode == 0, (text, done.stderr.decode()[-2000:])
    m = re.match(r"float_text_check: (\d+) patterns, (\d+) mismatches, longest text (\d+), multiword (\d+)\n$", text)
    assert m is not None, text
    assert int(m.group(1)) >= (1 << 32) // 4099 and int(m.group(2)) == 0 and int(m.group(3)) == 12 and int(m.group(4)) > 0


def test_exhaustive_run_is_recorded():
    text = open(os.path.join(xt.ROOT, "profiles", "float_text_exhaustive.txt")).read()
    assert "float_text_check --all: 4294967296 patterns, 0 mismatches, longest text 12" in text


def test_symbols_declared_bound_and_exported():
    import dliom
    header = open(os.path.join(xt.ROOT, "include", "dliom.h")).read()
    bound = {name for name, _, _ in dliom.SYMBOLS}
    L = dliom.load_library()
    for name in ("dliom_float_text", "dliom_points_batch_pack_xyz", "dliom_cloud_pack_xyz"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in bound
        assert getattr(L, name) is not None
    m = re.search(r"#define DLIOM_XYZ_MAX_RECORD (\d+)", header)
    assert m is not None and int(m.group(1)) == 39 == dliom.XYZ_MAX_RECORD == xt.MAX_RECORD
    for method in ("pack_xyz", "pack_xyz_size"):
        assert callable(getattr(dliom.PointsBatch, method))
    assert callable(dliom.PointCloud.pack_xyz)
    longest = b" ".join([dliom.float_text(-1.17549e-38)] * 3) + b"\n"
    assert len(longest) == dliom.XYZ_MAX_RECORD


def test_null_arguments_refused():
    import dliom
    L = dliom.load_library()
    buffer, n, size = C.create_string_buffer(16), C.c_int32(-7), C.c_int64(-7)
    assert L.dliom_float_text(C.c_float(1.5), None, C.byref(n)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_float_text(C.c_float(1.5), buffer, None) == dliom.ERR_INVALID_ARGUMENT
    assert n.value == -7 and buffer.raw == b"\0" * 16
    assert L.dliom_float_text(C.c_float(1.5), buffer, C.byref(n)) == dliom.OK and n.value == 3
    assert buffer.raw == b"1.5" + b"\0" * 13  # no terminator written: the rest is untouched
    assert L.dliom_points_batch_pack_xyz(None, None, 0, C.byref(size)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_pack_xyz(None, None, 0, C.byref(size)) == dliom.ERR_INVALID_ARGUMENT
