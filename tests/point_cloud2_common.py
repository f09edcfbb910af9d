"""Shared by the PointCloud2 tests: a numpy model of dliom.h "PointCloud2 messages decoded on the device" (structured views
of the message's bytes), random message layouts, and the driver of the one-thread C++ model (tests/cpp/point_cloud2_model.cc)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
OUSTER, VELODYNE, ROBOSENSE, OTHER, EXPORT, EXPORT_RSLIDAR = range(6)
MODES = (OUSTER, VELODYNE, ROBOSENSE, OTHER, EXPORT, EXPORT_RSLIDAR)
SLAM_MODES = (OUSTER, VELODYNE, ROBOSENSE, OTHER)
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)
NUMPY_TYPE = {INT8: "i1", UINT8: "u1", INT16: "<i2", UINT16: "<u2", INT32: "<i4", UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}
SIZE = {k: np.dtype(v).itemsize for k, v in NUMPY_TYPE.items()}
TIME_FIELD = {OUSTER: ("t", UINT32), VELODYNE: ("time", FLOAT32), ROBOSENSE: ("timestamp", FLOAT64)}
# a mount with a non-trivial rotation; the quaternion is NOT normalised once cast to float, like any real one
MOUNT = np.array([0.31, -0.12, 1.07, 0.8803, 0.1204, -0.3402, 0.3051])
f32 = np.float32


class Message:
    """sensor_msgs/PointCloud2 as plain data: fields is a list of (name, offset, datatype, count), data a uint8 array."""

    def __init__(self, height, width, point_step, row_step, fields, data, stamp_sec=0, stamp_nsec=0, is_bigendian=0, data_size=None):
        self.height, self.width, self.point_step, self.row_step = height, width, point_step, row_step
        self.fields, self.data, self.stamp_sec, self.stamp_nsec, self.is_bigendian = list(fields), data, stamp_sec, stamp_nsec, is_bigendian
        self.data_size = len(data) if data_size is None else data_size

    def to_library(self, dl):
        return dl.PointCloud2(self.height, self.width, self.point_step, self.row_step, self.fields, self.data, self.stamp_sec,
                              self.stamp_nsec, self.is_bigendian, self.data_size)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _find(m, name):
    for f in m.fields:
        if f[0] == name:
            return f
    return None


def _need(m, name, datatype):
    f = _find(m, name)
    return None if f is None or f[2] != datatype or f[3] != 1 else f[1]


def stamp_of(sec, nsec):
    return (sec + 719162 * 86400) * 10 ** 7 + (nsec + 50) // 100


def transform(pose7, xyz):
    """sensor_to_tracking.cast<float>() * p in float: Eigen's _transformVector order, then the translation"""
    t, (w, ux, uy, uz) = pose7[:3].astype(f32), pose7[3:].astype(f32)
    vx, vy, vz = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        ax, ay, az = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        ax, ay, az = ax + ax, ay + ay, az + az
        cx, cy, cz = uy * az - uz * ay, uz * ax - ux * az, ux * ay - uy * ax
        return np.stack([((vx + w * ax) + cx) + t[0], ((vy + w * ay) + cy) + t[1], ((vz + w * az) + cz) + t[2]], axis=1).astype(f32)


def ouster_seconds(u):
    """float(t) * 1e-9f: the uint32 to the nearest float, then a float product"""
    return u.astype(f32) * f32(1e-9)


def model_check(m, mode):
    """-> (status, plan): the refusals of dliom.h, the stamp and rel_time_last"""
    if mode not in MODES or m.is_bigendian != 0:
        return INVALID, None
    for name, offset, datatype, count in m.fields:
        if datatype not in SIZE or offset + SIZE[datatype] * count > m.point_step:
            return INVALID, None
    n = m.height * m.width
    if m.width * m.point_step > m.row_step or m.height * m.row_step > m.data_size or n >= 1 << 27:
        return INVALID, None
    plan = {"n": n, "time_field": None, "intensity": None, "rel_time_last": 0.0}
    for c in "xyz":
        if _need(m, c, FLOAT32) is None:
            return INVALID, None
    if mode in TIME_FIELD:
        name, datatype = TIME_FIELD[mode]
        if _need(m, name, datatype) is None or n == 0:
            return INVALID, None
        plan["time_field"] = name
    if mode == EXPORT:
        plan["intensity"] = "one"
        if _find(m, "intensity") is not None:
            if _need(m, "intensity", FLOAT32) is None:
                return INVALID, None
            plan["intensity"] = "field"
    if mode == EXPORT_RSLIDAR:
        if _need(m, "intensity", UINT8) is None:
            return INVALID, None
        plan["intensity"] = "field"
    plan["time"] = stamp_of(m.stamp_sec, m.stamp_nsec)
    if mode in TIME_FIELD:
        last = records(m)[plan["time_field"]][-1]
        rel = float(np.float64(ouster_seconds(np.array([last]))[0])) if mode == OUSTER else float(last)
        if not np.isfinite(rel) or not abs(rel * 1e7) < 2.0 ** 63:
            return INVALID, None
        plan["rel_time_last"] = rel
        if mode != ROBOSENSE:
            plan["time"] += int(rel * 1e7)  # truncates
    return OK, plan


def records(m):
    """the message's points as one structured array (a copy, in order), by structured views of each row's bytes"""
    names, seen = [], set()
    for f in m.fields:  # the first field of a name counts
        if f[0] not in seen and f[3] >= 1:
            seen.add(f[0])
            names.append(f)
    dt = np.dtype({"names": [f[0] for f in names], "formats": [NUMPY_TYPE[f[2]] for f in names], "offsets": [f[1] for f in names],
                   "itemsize": m.point_step})
    rows = [m.data[r * m.row_step: r * m.row_step + m.width * m.point_step].view(dt) for r in range(m.height)]
    return np.concatenate(rows) if rows else np.zeros(0, dt)


def model_decode(m, mode, sensor_to_tracking=None):
    """-> dict(status, xyzt, intensities (or None), time, origin, front, back)"""
    status, plan = model_check(m, mode)
    if status != OK:
        return {"status": status}
    r = records(m)
    n = plan["n"]
    xyz = np.stack([r["x"], r["y"], r["z"]], axis=1).astype(f32) if n else np.zeros((0, 3), f32)
    rel = np.float64(plan["rel_time_last"])
    if mode == OUSTER:
        t = (ouster_seconds(r["t"]).astype(np.float64) - rel).astype(f32)
    elif mode == VELODYNE:
        t = (r["time"].astype(np.float64) - rel).astype(f32)
    elif mode == ROBOSENSE:
        with np.errstate(all="ignore"):
            t = (r["timestamp"] - rel).astype(f32)
    else:
        t = np.zeros(n, f32)
    keep = np.isfinite(xyz).all(axis=1) if mode in SLAM_MODES else np.ones(n, bool)
    with np.errstate(all="ignore"):
        bad = ~(np.abs(t.astype(np.float64) * 1e7) < 2.0 ** 63)
    if (bad & keep).any():
        return {"status": INVALID}
    intensities = None
    if plan["intensity"] == "one":
        intensities = np.ones(n, f32)
    elif plan["intensity"] == "field":
        intensities = r["intensity"].astype(f32)
    origin = np.zeros(3, f32)
    if sensor_to_tracking is not None:
        xyz = transform(np.asarray(sensor_to_tracking, np.float64), xyz)
        origin = np.asarray(sensor_to_tracking[:3], np.float64).astype(f32)
    xyzt = np.concatenate([xyz, t.reshape(-1, 1)], axis=1)[keep]
    out = {"status": OK, "xyzt": np.ascontiguousarray(xyzt, f32), "intensities": None if intensities is None else intensities[keep],
           "time": plan["time"], "origin": origin, "rel_time_last": plan["rel_time_last"]}
    out["front"], out["back"] = (xyzt[0, 3], xyzt[-1, 3]) if len(xyzt) else (f32(0), f32(0))
    return out


# ---- messages ------------------------------------------------------------------------------------------------------------
def mode_fields(mode, with_intensity=True):
    """the fields a mode reads (name, datatype), then some it does not"""
    fields = [("x", FLOAT32), ("y", FLOAT32), ("z", FLOAT32)]
    if mode in TIME_FIELD:
        fields.append(TIME_FIELD[mode])
    if mode == EXPORT_RSLIDAR or (mode == ROBOSENSE and with_intensity):
        fields.append(("intensity", UINT8))
    elif with_intensity and mode != ROBOSENSE:
        fields.append(("intensity", FLOAT32))
    return fields


def pack_layout(rng, fields, point_step=None, shuffle=True, padding=True):
    """Offsets for the fields inside a record of point_step bytes (None: as small as they pack), in shuffled order with
    padding fields (a uint16 "ring", a uint8 x 3 "pad") in between where they fit; nothing is aligned on purpose."""
    fields = list(fields)
    if padding:
        fields += [("ring", UINT16, 1), ("pad", UINT8, 3)]
    fields = [f if len(f) == 3 else (f[0], f[1], 1) for f in fields]
    need = sum(SIZE[d] * c for name, d, c in fields if name not in ("ring", "pad"))
    if point_step is None:
        point_step = sum(SIZE[d] * c for _, d, c in fields)
    if shuffle:
        fields = [fields[k] for k in rng.permutation(len(fields))]
    while sum(SIZE[d] * c for _, d, c in fields) > point_step:  # drop padding fields until the rest fits
        victims = [k for k, f in enumerate(fields) if f[0] in ("ring", "pad")]
        if not victims:
            raise ValueError("point_step %d cannot hold %d bytes of fields" % (point_step, need))
        fields.pop(victims[0])
    slack = point_step - sum(SIZE[d] * c for _, d, c in fields)
    gaps = np.zeros(len(fields) + 1, int)
    for _ in range(slack):  # spread the slack in front of, between and behind the fields
        gaps[rng.randint(0, len(gaps))] += 1
    table, at = [], 0
    for k, (name, d, c) in enumerate(fields):
        at += gaps[k]
        table.append((name, int(at), d, c))
        at += SIZE[d] * c
    return table, point_step


def make_message(seed, mode, height, width, point_step=None, row_pad=0, odd_offset=True, with_intensity=True, shuffle=True,
                 stamp=(1_790_000_000, 123_456_789), time_span=0.1, absolute=1.6e9):
    """A random message for a mode: finite points in a 40 m box, times ascending to the last point (Ouster: ns from 0;
    Velodyne: s from 0; Robosense: absolute s near `absolute`), random bytes everywhere else."""
    rng = np.random.RandomState(seed)
    table, point_step = pack_layout(rng, mode_fields(mode, with_intensity), point_step, shuffle)
    row_step = width * point_step + row_pad
    n = height * width
    lead = 1 if odd_offset else 0
    big = rng.randint(0, 256, lead + height * row_step + 3).astype(np.uint8)
    data = big[lead: lead + height * row_step]
    m = Message(height, width, point_step, row_step, table, data, stamp[0], stamp[1])
    values = {"x": rng.uniform(-20, 20, n).astype(f32), "y": rng.uniform(-20, 20, n).astype(f32), "z": rng.uniform(-3, 8, n).astype(f32)}
    ramp = np.sort(rng.uniform(0, time_span, n))
    if mode == OUSTER:
        values["t"] = (ramp * 1e9).astype(np.uint32)
    elif mode == VELODYNE:
        values["time"] = ramp.astype(f32)
    elif mode == ROBOSENSE:
        values["timestamp"] = absolute + ramp
    f = _find(m, "intensity")
    if f is not None:
        values["intensity"] = rng.randint(0, 256, n).astype(np.uint8) if f[2] == UINT8 else rng.uniform(0, 255, n).astype(f32)
    set_values(m, values)
    return m


def set_values(m, values, index=None):
    """writes fields of the points `index` (None: all, in order) into the message's bytes"""
    idx = np.arange(m.height * m.width) if index is None else np.atleast_1d(index)
    if len(idx) == 0:
        return
    base =(idx // m.width) * m.row_step + (idx % m.width) * m.point_step
    for name, v in values.items():
        f = _find(m, name)
        raw = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=NUMPY_TYPE[f[2]]), idx.shape)).view(np.uint8).reshape(len(idx), -1)
        for b in range(raw.shape[1]):
            m.data[base + f[1] + b] = raw[:, b]


# ---- the C++ model as a program ------------------------------------------------------------------------------------------
def build_model(tmp_dir):
    exe = os.path.join(str(tmp_dir), "point_cloud2_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "point_cloud2_model.cc")])
    return exe


def run_model(exe, tmp_dir, cases):
    """cases: [(message, mode, sensor_to_tracking or None)] -> one dict a case, shaped like model_decode's"""
    src, dst = os.path.join(str(tmp_dir), "cases.bin"), os.path.join(str(tmp_dir), "results.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for m, mode, tf in cases:
            f.write(struct.pack("<ii7d", mode, 0 if tf is None else 1, *(np.zeros(7) if tf is None else tf)))
            f.write(struct.pack("<7Ii", m.height, m.width, m.point_step, m.row_step, m.is_bigendian, m.stamp_sec, m.stamp_nsec, len(m.fields)))
            for name, offset, datatype, count in m.fields:
                f.write(struct.pack("<32s3I", name.encode(), offset, datatype, count))
            used = min(m.data_size, len(m.data))
            f.write(struct.pack("<QQ", m.data_size if m.data_size <= len(m.data) else used, 1))
            f.write(m.data[:used].tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "POINT CLOUD2 MODEL DONE %d" % len(cases) in out.stdout, out.stdout + out.stderr
    raw = open(dst, "rb").read()
    results, at = [], 0
    for _ in cases:
        status, time, ox, oy, oz, kept, has = struct.unpack_from("<iq3fqi", raw, at)
        at += struct.calcsize("<iq3fqi")
        xyzt = np.frombuffer(raw, np.float32, 4 * kept, at).reshape(-1, 4)
        at += 16 * kept
        it = None
        if has:
            it = np.frombuffer(raw, np.float32, kept, at)
            at += 4 * kept
        r = {"status": status}
        if status == OK:
            r.update(xyzt=xyzt, intensities=it, time=time, origin=np.array([ox, oy, oz], f32))
            r["front"], r["back"] = (xyzt[0, 3], xyzt[-1, 3]) if kept else (f32(0), f32(0))
        results.append(r)
    assert at == len(raw)
    return results


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_equal_results(got, want, what=""):
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    if want["status"] != OK:
        return
    assert same_bits(got["xyzt"], want["xyzt"]), what
    assert (got["intensities"] is None) == (want["intensities"] is None), what
    if want["intensities"] is not None:
        assert same_bits(got["intensities"], want["intensities"]), what
    assert got["time"] == want["time"], (what, got["time"], want["time"])
    assert same_bits(got["origin"], want["origin"]), what
    assert same_bits([got["front"], got["back"]], [want["front"], want["back"]]), what


def layouts():
    """(name, height, width of n, point_step, row_pad) families the tests run every mode over: 22-byte Velodyne-like
    records, 26, 32, 48, the tightest packing, a padded row_step with height 4 (workgroup spans straddle row ends)."""
    return [("tight", 1, None, 0), ("h4_pad", 4, None, 7), ("step32", 1, 32, 0), ("step48_h4", 4, 48, 40), ("step26", 1, 26, 3)]


def smallest_step(mode):
    return sum(SIZE[d] for _, d in mode_fields(mode))


# ---- sensor-shaped messages of a scan (the front-end tests and tools/point_cloud2_bench.py) ---------------------------------
OUSTER_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 16, FLOAT32, 1), ("t", 20, UINT32, 1),
                 ("reflectivity", 24, UINT16, 1), ("ring", 26, UINT8, 1), ("ambient", 28, UINT16, 1), ("range", 32, UINT32, 1)]  # 48 bytes
VELODYNE_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 12, FLOAT32, 1),
                   ("ring", 16, UINT16, 1), ("time", 18, FLOAT32, 1)]  # 22 bytes: the time is not aligned


def scan_message(mode, points, rel_t, height, width, seed=0, stamp=(1_790_000_000, 500_000_000)):
    """An Ouster- (48 B) or Velodyne-shaped (22 B) message of height x width points of a scan: points (n, 3) and their times
    relative to the last one (ascending, <= 0) as the driver would send them -- nanoseconds, or seconds, since the first."""
    fields, step = (OUSTER_FIELDS, 48) if mode == OUSTER else (VELODYNE_FIELDS, 22)
    n = height * width
    rng = np.random.RandomState(seed)
    data = rng.randint(0, 256, n * step).astype(np.uint8)
    m = Message(height, width, step, width * step, fields, data, stamp[0], stamp[1])
    since_first = np.asarray(rel_t[:n], np.float64) - float(rel_t[0])
    values = {"x": points[:n, 0], "y": points[:n, 1], "z": points[:n, 2], "intensity": rng.uniform(0, 255, n).astype(f32)}
    if mode == OUSTER:
        values["t"] = np.round(since_first * 1e9).astype(np.uint32)
    else:
        values["time"] = since_first.astype(f32)
    set_values(m, values)
    return m
