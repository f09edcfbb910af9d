"""PointCloud2 decoding, the host half (no GPU): the numpy model and the one-thread C++ model of dliom.h's statement agree
bit for bit, the time arithmetic is the one the reference evaluates and not a neighbour of it, dliom_point_cloud2_check's
refusals and stamps, csrc/point_cloud2_layout.h under the sanitizers, and the header against the ctypes mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import point_cloud2_common as pc

f32 = np.float32


@pytest.fixture(scope="module")
def dl():
    import __graft_entry__
    __graft_entry__.build()
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("point_cloud2_model")
    return pc.build_model(d), d


def _random_cases():
    cases, seed = [], 0
    for mode in pc.MODES:
        for step in (16, 22, 26, 32, 48, None):
            for height in (1, 4):
                with_intensity = True
                if step == 16 and mode in (pc.OUSTER, pc.VELODYNE):
                    with_intensity = False  # x, y, z and the time fill 16 bytes
                if step == 16 and mode == pc.ROBOSENSE:
                    continue  # three floats and a double do not fit a 16-byte record
                seed += 1
                rng = np.random.RandomState(seed)
                m = pc.make_message(seed, mode, height, int(rng.randint(1, 40)), step, row_pad=int(rng.randint(0, 9)) if height > 1 else 0,
                                    with_intensity=with_intensity if mode != pc.EXPORT else seed % 2 == 0)  # EXPORT: with and without
                n = m.height * m.width
                bad = rng.randint(0, n, max(1, n // 6))  # some points a SLAM mode drops
                pc.set_values(m, {"xyz"[int(rng.randint(0, 3))]: rng.choice([np.nan, np.inf, -np.inf])}, bad[: len(bad) // 2 + 1])
                cases.append((m, mode, pc.MOUNT if seed % 3 else None))
    return cases


def test_the_two_models_agree(model):
    exe, d = model
    cases = _random_cases()
    assert len(cases) >= 60 and {c[0].point_step for c in cases} >= {16, 22, 26, 32, 48}
    got = pc.run_model(exe, d, cases)
    kept_some = dropped_some = 0
    for k, ((m, mode, tf), g) in enumerate(zip(cases, got)):
        want = pc.model_decode(m, mode, tf)
        assert want["status"] == pc.OK
        pc.assert_equal_results(g, want, "case %d mode %d step %d" % (k, mode, m.point_step))
        kept_some += len(want["xyzt"]) > 0
        dropped_some += len(want["xyzt"]) < m.height * m.width
    assert kept_some >= 50 and dropped_some >= 30


def test_the_two_models_agree_on_refusals(model):
    exe, d = model
    m = pc.make_message(5, pc.VELODYNE, 1, 9, 22)
    pc.set_values(m, {"time": np.nan}, 3)  # a kept point with a time the assembler would refuse
    late = pc.make_message(6, pc.VELODYNE, 1, 9, 22)
    pc.set_values(late, {"time": np.inf}, 8)  # rel_time_last
    cases = [(m, pc.VELODYNE, None), (late, pc.VELODYNE, None), (pc.make_message(7, pc.OTHER, 1, 5), pc.OUSTER, None)]
    for g, (msg, mode, tf) in zip(pc.run_model(exe, d, cases), cases):
        assert g["status"] == pc.INVALID and pc.model_decode(msg, mode, tf)["status"] == pc.INVALID


def test_time_arithmetic_is_the_references_and_no_neighbour_of_it():
    """Ouster: float(t) * 1e-9f in float, then double minus double.  Three plausible restatements give other floats on a
    quarter of the points or more, so a model (or a kernel) that took one of them would not pass the equality tests."""
    rng = np.random.RandomState(0)
    u = np.sort(rng.randint(0, 10 ** 8, 2048)).astype(np.uint32)
    inexact = np.mean(u.astype(f32).astype(np.int64) != u.astype(np.int64))
    m = pc.make_message(1, pc.OUSTER, 1, 2048, 48)
    pc.set_values(m, {"t": u})
    t = pc.model_decode(m, pc.OUSTER)["xyzt"][:, 3]
    rel = np.float64(pc.ouster_seconds(u[-1:])[0])
    all_double = (u.astype(np.float64) * 1e-9 - np.float64(u[-1]) * 1e-9).astype(f32)
    integer_first = ((u.astype(np.int64) - np.int64(u[-1])).astype(f32) * f32(1e-9)).astype(f32)
    # a fused multiply-subtract in double: the product of two floats is exact in double, so one rounding is left
    fused = (u.astype(f32).astype(np.float64) * np.float64(f32(1e-9)) - rel).astype(f32)
    shares = {"all-double": np.mean(t != all_double), "integer subtraction first": np.mean(t != integer_first),
              "product fused into the subtraction": np.mean(t != fused)}
    print("inexact in float: %.1f %%" % (100 * inexact))
    for name, share in shares.items():
        print("%s: differs on %.1f %% of the points" % (name, 100 * share))
    assert inexact >= 0.25
    for name, share in shares.items():
        assert share >= 0.25, (name, share)
    # Robosense: absolute stamps near 1.6e9 s, subtracted in double -- not cast to float first
    r = pc.make_message(2, pc.ROBOSENSE, 1, 2048, 32)
    stamps = pc.records(r)["timestamp"]
    t = pc.model_decode(r, pc.ROBOSENSE)["xyzt"][:, 3]
    cast_first = stamps.astype(f32) - f32(stamps[-1])
    share = np.mean(t[:-1] != cast_first[:-1])
    print("Robosense, cast to float then subtract: differs on %.1f %% of the points" % (100 * share))
    assert share >= 0.90


def _status(dl, m, mode):
    return m.to_library(dl).check(mode)[0]


def test_check_refusals(dl):
    good = pc.make_message(3, pc.VELODYNE, 2, 6, 26, row_pad=5)
    assert _status(dl, good, pc.VELODYNE) == pc.OK

    def changed(mode=pc.VELODYNE, seed=3, **kw):
        m = pc.make_message(seed, mode, 2, 6, 26 if mode != pc.ROBOSENSE else 32, row_pad=5)  # (every padding field fits)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def refield(m, which, **kw):
        m.fields = [tuple(kw.get(key, old) for key, old in zip(("name", "offset", "datatype", "count"), f)) if f[0] == which else f
                    for f in m.fields]
        return m

    refused = {
        "big-endian": (changed(is_bigendian=1), pc.VELODYNE),
        "x missing": (refield(changed(), "x", name="u"), pc.VELODYNE),
        "y of another datatype": (refield(changed(), "y", datatype=pc.INT32), pc.VELODYNE),
        "z with count 2": (refield(changed(), "z", count=2, offset=0), pc.VELODYNE),
        "time missing": (changed(pc.OTHER), pc.VELODYNE),
        "Ouster's t as a float": (refield(changed(pc.OUSTER), "t", datatype=pc.FLOAT32), pc.OUSTER),
        "Robosense's timestamp as a float": (refield(changed(pc.ROBOSENSE), "timestamp", datatype=pc.FLOAT32), pc.ROBOSENSE),
        "export: intensity of another datatype": (refield(changed(pc.EXPORT), "intensity", datatype=pc.UINT32), pc.EXPORT),
        "export rslidar: float intensity": (changed(pc.EXPORT), pc.EXPORT_RSLIDAR),
        "a datatype outside 1 .. 8": (refield(changed(), "ring", datatype=9), pc.VELODYNE),
        "a field past the record": (refield(changed(), "time", offset=23), pc.VELODYNE),
        "a count that overflows 32 bits": (refield(changed(), "ring", count=0xFFFFFFFF), pc.VELODYNE),
        "width * point_step > row_step": (changed(row_step=6 * 26 - 1), pc.VELODYNE),
        "height * row_step > data_size": (changed(data_size=2 * (6 * 26 + 5) - 1), pc.VELODYNE),
        "an empty message in a timed mode": (changed(height=0), pc.VELODYNE),
    }
    for what, (m, mode) in refused.items():
        assert _status(dl, m, mode) == dl.ERR_INVALID_ARGUMENT, what
        assert pc.model_check(m, mode)[0] == pc.INVALID, what
    assert _status(dl, changed(pc.OTHER, height=0), pc.OTHER) == pc.OK  # the untimed modes take it
    # n >= 2^27: no byte is read before the refusal (the sizes alone say it)
    xyz_only = [("x", 0, pc.FLOAT32, 1), ("y", 4, pc.FLOAT32, 1), ("z", 8, pc.FLOAT32, 1)]
    huge = pc.Message(1 << 14, 1 << 13, 16, 16 << 13, xyz_only, good.data, data_size=16 << 27)
    assert _status(dl, pc.Message(1, 4, 16, 64, xyz_only, good.data), pc.OTHER) == pc.OK
    assert _status(dl, huge, pc.OTHER) == dl.ERR_INVALID_ARGUMENT
    # a rel_time_last that is not finite
    for value in (np.nan, np.inf, -np.inf):
        m = changed()
        pc.set_values(m, {"time": value}, 11)
        assert _status(dl, m, pc.VELODYNE) == dl.ERR_INVALID_ARGUMENT
        pc.set_values(m, {"time": 0.25}, 11)
        pc.set_values(m, {"time": value}, 4)  # not the last point: the check does not look at it
        assert _status(dl, m, pc.VELODYNE) == pc.OK
    r = changed(pc.ROBOSENSE)
    pc.set_values(r, {"timestamp": np.nan}, 11)
    assert _status(dl, r, pc.ROBOSENSE) == dl.ERR_INVALID_ARGUMENT
    L = dl.load_library()
    assert L.dliom_point_cloud2_check(None, 0, None, None) == dl.ERR_INVALID_ARGUMENT
    assert good.to_library(dl).check(6)[0] == dl.ERR_INVALID_ARGUMENT and good.to_library(dl).check(-1)[0] == dl.ERR_INVALID_ARGUMENT


def test_check_stamp(dl):
    m = pc.make_message(4, pc.OTHER, 1, 3)
    for nsec in (0, 49, 50, 149, 999_999_949, 999_999_999):
        m.stamp_sec, m.stamp_nsec = 1_790_000_000, nsec
        status, time, rel = m.to_library(dl).check(pc.OTHER)
        want = (1_790_000_000 + 719162 * 86400) * 10 ** 7 + (nsec + 50) // 100
        assert (status, time, rel) == (pc.OK, want, 0.0) and pc.model_check(m, pc.OTHER)[1]["time"] == want
    assert pc.stamp_of(0, 49) - pc.stamp_of(0, 0) == 0 and pc.stamp_of(0, 50) - pc.stamp_of(0, 0) == 1
    assert pc.stamp_of(0, 999_999_999) == pc.stamp_of(1, 0)
    # FromSeconds(rel_time_last) truncates: 0.09999996 s is 999 999.6 ticks
    v = pc.make_message(5, pc.VELODYNE, 1, 4, 22, stamp=(1_790_000_000, 0))
    last = f32(0.09999996)
    pc.set_values(v, {"time": last}, 3)
    ticks = float(last) * 1e7
    assert ticks - int(ticks) > 0.5  # rounding would give the next tick
    status, time, rel = v.to_library(dl).check(pc.VELODYNE)
    assert status == pc.OK and rel == float(last) and time == pc.stamp_of(1_790_000_000, 0) + int(ticks)
    assert pc.model_check(v, pc.VELODYNE)[1]["time"] == time
    # Ouster moves the stamp by its float product; Robosense's stamp stays
    o = pc.make_message(6, pc.OUSTER, 1, 4, 48, stamp=(1_790_000_000, 0))
    pc.set_values(o, {"t": np.uint32(99_999_999)}, 3)
    status, time, rel = o.to_library(dl).check(pc.OUSTER)
    assert rel == float(f32(99_999_999) * f32(1e-9)) and time == pc.stamp_of(1_790_000_000, 0) + int(rel * 1e7)
    r = pc.make_message(7, pc.ROBOSENSE, 1, 4, 32, stamp=(1_600_000_000, 7))
    status, time, rel = r.to_library(dl).check(pc.ROBOSENSE)
    assert status == pc.OK and time == pc.stamp_of(1_600_000_000, 7) and rel == pc.records(r)["timestamp"][-1]


def test_library_check_equals_model_on_random_messages(dl):
    for m, mode, _ in _random_cases():
        status, time, rel = m.to_library(dl).check(mode)
        want_status, plan = pc.model_check(m, mode)
        assert status == want_status == pc.OK and time == plan["time"] and rel == plan["rel_time_last"]


def test_layout_header_under_sanitizers(tmp_path):
    check = str(tmp_path / "point_cloud2_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", check,
                           os.path.join(pc.ROOT, "tests", "cpp", "point_cloud2_layout_check.cc")])
    accepted = 0
    for seed in (1, 2):
        out = subprocess.run([check, "4000", str(seed)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        a, r = (int(v) for v in re.match(r"accepted (\d+) refused (\d+)", out.stdout).groups())
        assert a + r == 4000 and r >= 1000
        accepted += a
    assert accepted >= 300  # the plans' own invariants were checked on these


def test_symbols_and_struct_layout(dl, tmp_path):
    header = open(os.path.join(pc.ROOT, "include", "dliom.h")).read()
    bound = {name for name, _, _ in dl.SYMBOLS}
    for name in ("dliom_point_cloud2_check", "dliom_point_cloud2_decode", "dliom_timed_cloud_destroy", "dliom_timed_cloud_size",
                 "dliom_timed_cloud_has_intensities", "dliom_timed_cloud_front_back_time", "dliom_timed_cloud_download",
                 "dliom_add_range_data_timed_cloud", "dliom_points_batch_from_timed_cloud"):
        assert name in bound and re.search(r"\b%s\(" % name, header), name
        assert hasattr(C.CDLL(dl.LIB_PATH), name)
    assert "parity unpinned against pcl" in header.lower()
    for k, name in enumerate(("SLAM_OUSTER", "SLAM_VELODYNE", "SLAM_ROBOSENSE", "SLAM_OTHER", "EXPORT", "EXPORT_RSLIDAR")):
        assert re.search(r"DLIOM_POINT_CLOUD2_%s = %d\b" % (name, k), header) and getattr(dl, "POINT_CLOUD2_" + name) == k
    src = tmp_path / "size.c"
    members = ("width", "row_step", "is_bigendian", "num_fields", "fields", "data", "data_size", "stamp_sec", "stamp_nsec")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dliom.h"\nint main(void) { printf("%zu %zu %zu %zu %zu '
                   + "%zu " * len(members) + '\\n", sizeof(dliom_point_field), offsetof(dliom_point_field, offset), '
                   "offsetof(dliom_point_field, datatype), offsetof(dliom_point_field, count), sizeof(dliom_point_cloud2), "
                   + ", ".join("offsetof(dliom_point_cloud2, %s)" % m for m in members) + "); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(pc.ROOT, "include"), "-o", str(exe), str(src)])
    F, M = dl.PointField, dl.PointCloud2Struct
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == \
        [C.sizeof(F), F.offset.offset, F.datatype.offset, F.count.offset, C.sizeof(M)] + [getattr(M, m).offset for m in members]


def test_argument_checks_without_a_context(dl):
    L = dl.load_library()
    m = pc.make_message(8, pc.OTHER, 1, 3).to_library(dl)
    h, t, o = C.c_void_p(), C.c_int64(), np.zeros(3, f32)
    assert L.dliom_point_cloud2_decode(None, C.byref(m.struct), pc.OTHER, None, C.byref(h), C.byref(t),
                                       o.ctypes.data_as(C.POINTER(C.c_float))) == dl.ERR_INVALID_ARGUMENT
    n = C.c_int64()
    assert L.dliom_timed_cloud_size(None, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_timed_cloud_destroy(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_timed_cloud_download(None, None, None) == dl.ERR_INVALID_ARGUMENT
