"""Shared by tests/test_xyz_text_host.py, tests/test_gpu_xyz_text.py and tools/xyz_bench.py: builds and runs the CPU model
of the XYZ writer (tests/cpp/xyz_writer_model.cc: the reference's std::ostringstream loop), the stand-alone check of
csrc/float_text.h (tests/cpp/float_text_check.cc) and the adapter program, and makes the inputs."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "xyz_writer_model.cc")
CHECK_SRC = os.path.join(ROOT, "tests", "cpp", "float_text_check.cc")
ADAPTER_SRC = os.path.join(ROOT, "tests", "cpp", "xyz_writer_adapter.cc")
f32 = np.float32
MAX_RECORD = 39
TEXT_POINTS = 256  # points a workgroup formats (points_text.hip)


def build_model(directory):
    exe = os.path.join(str(directory), "xyz_writer_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def run_model(exe, points, directory, timing=False):
    """points (n, 3) float32 -> the text the reference's loop writes (bytes)[, its milliseconds]."""
    src, dst = os.path.join(str(directory), "xyz_in.bin"), os.path.join(str(directory), "xyz_out.txt")
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(points, dtype=f32).tobytes())
    text = subprocess.check_output([exe, src, dst] + (["--time"] if timing else [])).decode()
    data = open(dst, "rb").read()
    return (data, float(text)) if timing else data


def model_texts(exe, values, directory):
    """values float32 (k,) -> [bytes] * k: each value's text, through the model (as the x of a point 'v 0 0')."""
    values = np.ascontiguousarray(values, dtype=f32).reshape(-1)
    pts = np.zeros((len(values), 3), dtype=f32)
    pts[:, 0] = values
    lines = run_model(exe, pts, directory).split(b"\n")
    assert lines[-1] == b"" and len(lines) == len(values) + 1
    out = []
    for line in lines[:-1]:
        assert line.endswith(b" 0 0")
        out.append(line[:-4])
    return out


def build_check(directory, sanitize):
    """The stand-alone check of float_text.h, plain or with -fsanitize=address,undefined (its own main: nothing preloaded)."""
    exe = os.path.join(str(directory), "float_text_check_san" if sanitize else "float_text_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread"] + flags +
                          ["-I", os.path.join(ROOT, "d-liom_amd", "csrc"), "-o", exe, CHECK_SRC])
    return exe


def python_text(value):
    """'%.6g' of the promoted float with the C library's spelling of the sign of a NaN."""
    v = f32(value)
    if np.isnan(v):
        return b"-nan" if (v.view(np.uint32) >> 31) else b"nan"
    return ("%.6g" % float(v)).encode()


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).astype(np.uint32).view(f32)


def special_values():
    """zeros, infinities, NaNs of both signs (quiet, signalling-pattern, full payload), the extremes of the format"""
    return from_bits([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001,
                      0x7fffffff, 0xffffffff, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x80800000, 0x7f7fffff,
                      0xff7fffff, 0x3f800000, 0xbf800000])


def exponent_field_values(seed=11):
    """every exponent field x both signs x mantissas {0, 1, 2, 0x400000, 0x7ffffe, 0x7fffff, 64 random}"""
    rng = np.random.RandomState(seed)
    bits = []
    for field in range(256):
        mantissas = [0, 1, 2, 0x400000, 0x7ffffe, 0x7fffff] + [int(m) for m in rng.randint(0, 1 << 23, size=64)]
        for sign in (0, 1):
            bits += [(sign << 31) | (field << 23) | m for m in mantissas]
    return from_bits(bits)


def _neighbours(values64):
    """the floats next to each double: the nearest float and both its float neighbours, finite and positive only"""
    out = []
    for v in values64:
        with np.errstate(over="ignore", under="ignore"):
            c = f32(v)
        for w in (np.nextafter(c, f32(0)), c, np.nextafter(c, f32(np.inf))):
            if np.isfinite(w) and w > 0:
                out.append(w)
    return np.array(out, dtype=f32)


def decade_values():
    """both float neighbours of 10^k and of 999999.5 * 10^(k - 5), for every k the format reaches (-45 .. 38)"""
    ks = range(-46, 40)
    return _neighbours([float("1e%d" % k) for k in ks] + [float("9.999995e%d" % k) for k in ks])


NAMED_TIES = [1000.125, 100.0625, 10.03125, 1.015625, 100000.5, 100001.5, 1234565.0]
# (value, text): the named ties spelled out, so that the reference itself is pinned
NAMED_TEXTS = [(1000.125, b"1000.12"), (100.0625, b"100.062"), (10.03125, b"10.0312"), (1.015625, b"1.01562"),
               (100000.5, b"100000"), (100001.5, b"100002"), (1234565.0, b"1.23456e+06")]


def tie_values(seed=12, per_decade=200):
    """(2 D + 1) * 10^(X - 5) / 2 rounded to float for X in -3 .. 6, D random in [10^5, 10^6): where the value is a float
    it is an exact tie between two six-digit texts; the named ones first."""
    rng = np.random.RandomState(seed)
    out = [f32(v) for v in NAMED_TIES]
    for x in range(-3, 7):
        for d in rng.randint(100000, 1000000, size=per_decade):
            out.append(f32((2 * int(d) + 1) * 10.0 ** (x - 5) / 2.0))
        # The exact ties among them.  X <= 5: (2 D + 1) / (2^(6 - X) * 5^(5 - X)) is a float exactly when 5^(5 - X) divides
        # 2 D + 1 = k * 5^(5 - X), k odd, and then it is k / 2^(6 - X) (k < 2^21).  X = 6: (2 D + 1) * 5 < 2^24, an integer.
        if x == 6:
            out += [f32((2 * int(d) + 1) * 5) for d in rng.randint(100000, 1000000, size=per_decade)]
            continue
        p5 = 5 ** (5 - x)
        ks = [k for k in range(200001 // p5 + 1, 2000000 // p5 + 1) if k % 2 == 1 and 200001 <= k * p5 < 2000000]
        for k in (ks if len(ks) <= per_decade else [ks[int(j)] for j in rng.randint(0, len(ks), size=per_decade)]):
            out.append(f32(k / 2.0 ** (6 - x)))
    out = np.array(out, dtype=f32)
    return np.concatenate([out, -out])


def stride_points(count=1 << 20, stride=1367, start=12345):
    """`count` points whose 3 * count coordinates are the bit patterns start + i * stride (mod 2^32): with stride = 1367
    (a prime near 2^32 / (3 * 2^20)) they run once through all 2^32."""
    i = np.arange(3 * count, dtype=np.uint64)
    bits = ((np.uint64(start) + i * np.uint64(stride)) & np.uint64(0xffffffff)).astype(np.uint32)
    return bits.view(f32).reshape(count, 3)


def as_axis(values, axis):
    """points with `values` on one axis and short ordinary numbers on the others"""
    values = np.ascontiguousarray(values, dtype=f32).reshape(-1)
    pts = np.empty((len(values), 3), dtype=f32)
    pts[:] = np.array([1.5, -2.25, 3.0], dtype=f32)
    pts[:, axis] = values
    return pts


SHORT, LONG = (0.0, 0.0, 0.0), (-1.17549e-38, -1.17549e-38, -1.17549e-38)  # 6 and 39 bytes a record


def length_pattern(n, kind):
    """n points of 6-byte and 39-byte records: "short", "long", "by_point" (alternating) or "by_workgroup"."""
    i = np.arange(n)
    long_one = {"short": np.zeros(n, bool), "long": np.ones(n, bool), "by_point": i % 2 == 1,
                "by_workgroup": (i // TEXT_POINTS) % 2 == 1}[kind]
    pts = np.empty((n, 3), dtype=f32)
    pts[~long_one] = np.array(SHORT, dtype=f32)
    pts[long_one] = np.array(LONG, dtype=f32)
    return pts


def build_adapter(directory, lib_path):
    exe = os.path.join(str(directory), "xyz_writer_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "d-liom_amd", "cpp"), "-o", exe, ADAPTER_SRC, lib_path,
                           "-Wl,-rpath," + os.path.dirname(lib_path)])
    return exe


def run_adapter(exe, directory, times, poses, mount, messages, min_range=1.0, max_range=20.0):
    """messages: [(cloud_time, xyzt, intensities, frame_id)] -> dict: device / host (file bytes, counted points), uploads,
    downloaded"""
    src, dst = os.path.join(str(directory), "xyz_pipeline_in.bin"), os.path.join(str(directory), "xyz_pipeline_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(times)) + np.ascontiguousarray(times, dtype=np.int64).tobytes())
        f.write(np.ascontiguousarray(poses, dtype=np.float64).tobytes() + np.ascontiguousarray(mount, dtype=np.float64).tobytes())
        f.write(struct.pack("<q", len(messages)))
        for cloud_time, xyzt, intensities, frame_id in messages:
            name = frame_id.encode()
            f.write(struct.pack("<qqq", int(cloud_time), len(xyzt), len(name)) + name)
            f.write(np.ascontiguousarray(xyzt, dtype=f32).tobytes())
            f.write(np.ascontiguousarray(intensities, dtype=f32).tobytes())
    subprocess.run([exe, src, dst, repr(float(min_range)), repr(float(max_range))], timeout=300, check=True)
    data = open(dst, "rb").read()
    at, out = 0, {}
    for name in ("device", "host"):
        n, count = struct.unpack_from("<qq", data, at)
        out[name] = (data[at + 16:at + 16 + n], count)
        at += 16 + n
    out["uploads"], out["downloaded"] = struct.unpack_from("<qq", data, at)
    assert at + 16 == len(data)
    return out
