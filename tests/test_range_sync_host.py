"""Two range sensors' clouds merged on the device, the host half (no GPU): the numpy model of tests/range_sync_common.py
equals the adapter's host RangeDataSynchronizer (d-liom_amd/cpp/dliom_cartographer.h, driven by tests/cpp/synchronizer_cpu.cc)
bit for bit and in the same order on inputs full of equal times, the adapter header still compiles as C++11, and the new
entry points refuse missing arguments before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import range_sync_common as rs

f32 = np.float32


@pytest.fixture(scope="module")
def dl():
    import __graft_entry__
    __graft_entry__.build()
    import dliom
    dliom.load_library()
    return dliom


def _call(sensor_id, time, descrew, origin, xyzt):
    head = "%s %d %d %.9g %.9g %.9g %d" % (sensor_id, time, descrew, origin[0], origin[1], origin[2], len(xyzt))
    return head + "".join(" %.9g" % v for v in np.asarray(xyzt, f32).reshape(-1)) + "\n"


def test_model_equals_the_adapters_host_synchronizer(dl, orc, tmp_path):
    exe = str(tmp_path / "synchronizer_cpu")
    libdir = os.path.join(rs.ROOT, "d-liom_amd")
    # -std=c++11: the device overload must not cost the header its C++11 callers
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-o", exe, os.path.join(rs.ROOT, "tests", "cpp", "synchronizer_cpu.cc"),
                           "-I", os.path.join(rs.ROOT, "include"), "-I", os.path.join(libdir, "cpp"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
    origin_a, origin_b = (0.5, 0.0, 1.0), (-0.5, 0.25, 1.5)
    cases = [(m, pattern, descrew) for m in (17, 1000, 5000) for pattern in ("runs of 64", "all equal") for descrew in (0, 1)]
    cases.append((3000, "distinct", 0))
    script, want = "", []
    for k, (m, pattern, descrew) in enumerate(cases):
        primary, pt, secondary, st = rs.pair_of_merged_size(100 + k, m, pattern)
        shift = k * 10 ** 7  # a second between the pairs: the earlier secondary cloud is dropped as too old
        script += _call("lidar_b", st + shift, descrew, origin_b, secondary) + _call("lidar_a", pt + shift, descrew, origin_a, primary)
        if descrew:
            merged = rs.merge(orc, primary, pt + shift, rs.stamp(secondary, 0.1), st + shift, primary_for_times=rs.stamp(primary, 0.1))
        else:
            merged = rs.merge(orc, primary, pt + shift, secondary, st + shift)
        assert merged is not None
        if pattern != "distinct" and m >= 1000 and not descrew:
            t = merged[0][:, 3]
            assert np.max(np.bincount(np.unique(t, return_inverse=True)[1])) >= 64
        want.append((pt + shift, merged))
    out = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SYNCHRONIZER DONE" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    results, rows = [], None
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "RESULT":
            rows = []
            results.append((int(f[1]), int(f[2]), rows))
        elif f[0] == "R":
            rows.append([int(v) for v in f[1:6]])
    assert len(results) == 2 * len(cases)
    for k, (time, (xyzt, origin)) in enumerate(want):
        assert results[2 * k][1:] == (0, [])  # the secondary cloud waits
        got_time, got_origins, got_rows = results[2 * k + 1]
        got = np.array(got_rows, dtype=np.int64).reshape(-1, 5)
        assert (got_time, got_origins, len(got)) == (time, 2, len(xyzt)), cases[k]
        assert np.array_equal(got[:, 0], origin.astype(np.int64)), cases[k]
        assert np.array_equal(got[:, 1:].astype(np.uint32), xyzt.view(np.uint32)), cases[k]


def test_new_entry_points_refuse_missing_arguments(dl):
    """no context, no object: DLIOM_ERR_INVALID_ARGUMENT from every new entry point, *out left NULL -- nothing runs, and
    nothing pretends to have run, where there is no device to make a context on"""
    L = dl.load_library()
    out, has, k = C.c_void_p(), C.c_int(7), C.c_int(7)
    pose = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    zeros = (C.c_float * 8)()
    assert L.dliom_timed_cloud_stamp(None, None, 0.1, C.byref(out)) == dl.ERR_INVALID_ARGUMENT and not out
    assert L.dliom_timed_cloud_stamp(None, None, 0.1, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_timed_clouds_merge(None, None, None, 0, None, 0, C.byref(out)) == dl.ERR_INVALID_ARGUMENT and not out
    assert L.dliom_timed_clouds_merge(None, None, None, 0, None, 0, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_timed_cloud_has_origin_index(None, C.byref(has)) == dl.ERR_INVALID_ARGUMENT and has.value == 7
    assert L.dliom_timed_cloud_download_origin_index(None, zeros) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_range_accumulator_add_timed_cloud(None, pose, pose, 0.1, None, zeros, 1, 1.0, 60.0, 0.15, zeros,
                                                     C.byref(k)) == dl.ERR_INVALID_ARGUMENT and k.value == 7


def test_symbols_are_declared_bound_and_exported(dl):
    header = open(os.path.join(rs.ROOT, "include", "dliom.h")).read()
    bound = {name for name, _, _ in dl.SYMBOLS}
    for name in ("dliom_timed_cloud_has_origin_index", "dliom_timed_cloud_download_origin_index", "dliom_timed_cloud_stamp",
                 "dliom_timed_clouds_merge", "dliom_range_accumulator_add_timed_cloud"):
        assert name in bound and re.search(r"\b%s\(" % name, header), name
        assert hasattr(C.CDLL(dl.LIB_PATH), name)
    for name in ("merge_timed_clouds",):
        assert callable(getattr(dl, name))
    assert callable(dl.TimedCloud.stamp) and callable(dl.RangeDataAccumulator.add_timed_cloud)
