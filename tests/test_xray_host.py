"""X-ray projections (dliom_grid_xray_texture, dliom_grid_project_to_image) without a GPU: the names are bound, the
argument checks refuse before anything runs, the host log-odds table equals ProbabilityToLogOddsInteger for every float
in [0.1, 0.9], and the CPU model (tests/cpp/xray_model.cc) gives hand-computed pixels on tiny grids."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "xray_model.cc")
f32 = np.float32


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xray_model") / "xray_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


# ---- helpers shared with tests/test_gpu_xray.py ---------------------------------------------------------------------
def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def grid_proto(resolution, cells):
    """Serialized mapping::proto::HybridGrid of (x, y, z, value) cells, which must be listed in iterator order."""
    def packed(field, values):
        payload = b"".join(_varint(v) for v in values)
        return _varint(field << 3 | 2) + _varint(len(payload)) + payload if payload else b""
    zz = lambda n: ((n << 1) ^ (n >> 31)) & 0xFFFFFFFF
    out = b"\x0d" + struct.pack("<f", resolution)
    for k in range(3):
        out += packed(3 + k, [zz(c[k]) for c in cells])
    return out + packed(6, [c[3] for c in cells])


def run_model(exe, mode, proto, pose, tmp_path):
    src, dst = tmp_path / "grid.pb", tmp_path / "out.bin"
    src.write_bytes(proto)
    subprocess.check_call([exe, mode, str(src)] + [repr(float(v)) for v in pose] + [str(dst)])
    data = dst.read_bytes()
    w, h, res = struct.unpack_from("<iid", data)
    if mode == "texture":
        slice_pose = np.array(struct.unpack_from("<7d", data, 16))
        cells = np.frombuffer(data[72:], dtype=np.uint8).reshape(h, w, 2)
        return w, h, res, slice_pose, cells
    ox, oy = struct.unpack_from("<2d", data, 16)
    return np.frombuffer(data[32:], dtype=np.uint8).reshape(h, w), ox, oy, res


# ---- float32 restatement of the few formulas the expected pixels need ------------------------------------------------
P_MIN, P_MAX = f32(0.1), f32(1) - f32(0.1)


def v2p(v):
    scale = (P_MAX - P_MIN) / f32(32766)
    return f32(f32(v) * scale) + (P_MIN - scale)


def lround(x):
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def image_byte(values):
    s = f32(0)
    for v in values:
        s = f32(s + v2p(v))
    return lround(f32(f32(s - P_MIN) * f32(f32(255) / (P_MAX - P_MIN)))) % 256


def texture_pixel(dl, values, zs):
    count, zd = len(values), f32(max(zs) - min(zs))
    if zd < f32(3):
        return 0, 0
    s, maxp = f32(0), f32(0.5)
    for v in values:
        s = f32(s + v2p(v))
        maxp = max(maxp, v2p(v))
    free = max(f32(zd - f32(count)), f32(0))
    fsw = f32(f32(0.15) * free)
    avg = f32(f32(s + f32(f32(1) - maxp) * fsw) / f32(f32(count) + fsw))
    avg = min(max(avg, P_MIN), P_MAX)
    delta = 128 - dl.probability_to_log_odds_integer(avg)
    value, alpha = (delta, 0) if delta > 0 else (0, -delta)
    return value, (alpha if value or alpha else 1)


IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


# ---- the library without a GPU --------------------------------------------------------------------------------------
def test_xray_symbols_exported(dl):
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("dliom_grid_xray_texture", "dliom_grid_project_to_image", "dliom_probability_to_log_odds_integer"):
        assert n in names
        assert getattr(dl.load_library(), n) is not None


def test_xray_argument_checks(dl):
    L = dl.load_library()
    pose = (C.c_double * 7)(*IDENTITY)
    sl = (C.c_double * 7)()
    w, h = C.c_int32(), C.c_int32()
    res, ox, oy = C.c_double(), C.c_double(), C.c_double()
    bad = dl.ERR_INVALID_ARGUMENT
    assert L.dliom_grid_xray_texture(None, pose, None, 0, C.byref(w), C.byref(h), C.byref(res), sl) == bad
    assert L.dliom_grid_xray_texture(None, None, None, 0, C.byref(w), C.byref(h), C.byref(res), sl) == bad
    assert L.dliom_grid_project_to_image(None, pose, None, 0, C.byref(w), C.byref(h), C.byref(ox), C.byref(oy),
                                         C.byref(res)) == bad
    assert L.dliom_grid_project_to_image(None, None, None, 0, C.byref(w), C.byref(h), C.byref(ox), C.byref(oy),
                                         C.byref(res)) == bad


def test_log_odds_table_equals_formula_for_every_float(dl, tmp_path):
    """dliom_probability_to_log_odds_integer == RoundToInt((Logit(p) - kMinLogOdds) * 254 / (kMax - kMin)) + 1 with
    glibc's logf, for all ~25 M floats in [0.1, 0.9]; the formula is monotone there and covers 1..255."""
    exe = str(tmp_path / "log_odds_exhaustive")
    libdir = os.path.join(ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-DXRAY_MODEL_EXHAUSTIVE",
                           "-o", exe, MODEL_SRC, "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "first 1 last 255" in r.stdout, r.stdout
    assert dl.probability_to_log_odds_integer(0.5) == 128


def test_model_one_cell(dl, model, tmp_path):
    v = int(dl.load_library().dliom_probability_to_value(C.c_float(0.6)))
    proto = grid_proto(0.1, [(2, -3, 1, v)])
    w, h, res, slice_pose, cells = run_model(model, "texture", proto, IDENTITY, tmp_path)
    assert (w, h, res) == (1, 1, float(f32(0.1)))
    assert cells.tolist() == [[[0, 0]]]  # a single cell has no z extent
    assert slice_pose.tolist() == [float(f32(2) * f32(0.1)), float(f32(-3) * f32(0.1)), 0.0, 1.0, 0.0, 0.0, 0.0]
    img, ox, oy, res = run_model(model, "image", proto, IDENTITY, tmp_path)
    assert img.tolist() == [[image_byte([v])]]
    assert (ox, oy) == (2 * float(f32(0.1)), -3 * float(f32(0.1)))


def test_model_column_below_and_above_min_z_difference(dl, model, tmp_path):
    L = dl.load_library()
    va, vb, vc = (int(L.dliom_probability_to_value(C.c_float(p))) for p in (0.55, 0.7, 0.9))
    low = grid_proto(0.1, [(0, 0, 0, va), (0, 0, 1, vb), (0, 0, 2, vc)])  # z extent 2 < kMinZDifference
    assert run_model(model, "texture", low, IDENTITY, tmp_path)[4].tolist() == [[[0, 0]]]
    high = grid_proto(0.1, [(0, 0, 0, va), (0, 0, 1, vb), (0, 0, 3, vc)])  # z extent 3: counted
    px = texture_pixel(dl, [va, vb, vc], [0, 1, 3])
    assert px != (0, 0)
    assert run_model(model, "texture", high, IDENTITY, tmp_path)[4].tolist() == [[list(px)]]
    gap = grid_proto(0.1, [(0, 0, 0, va), (0, 0, 4, vb)])  # free space between: weight 0.15 * 2, 1 - max probability
    assert run_model(model, "texture", gap, IDENTITY, tmp_path)[4].tolist() == [[list(texture_pixel(dl, [va, vb], [0, 4]))]]
    img = run_model(model, "image", high, IDENTITY, tmp_path)[0]
    assert img.tolist() == [[image_byte([va, vb, vc])]]


def test_model_negative_indices_across_meta_cells(dl, model, tmp_path):
    """Cells at x = -1 (meta cell -1) and x = 0 (meta cell 0): texture rows run from max_x down, image columns from min_x up."""
    L = dl.load_library()
    va, vb = (int(L.dliom_probability_to_value(C.c_float(p))) for p in (0.6, 0.8))
    cells = [(-1, 0, z, va) for z in (0, 1, 2, 3)] + [(0, 0, 0, vb), (0, 0, 5, vb)]  # iterator order: meta x -1 first
    proto = grid_proto(0.1, cells)
    w, h, _, slice_pose, tex = run_model(model, "texture", proto, IDENTITY, tmp_path)
    assert (w, h) == (1, 2)
    assert tex[0, 0].tolist() == list(texture_pixel(dl, [vb, vb], [0, 5]))  # row max_x - 0
    assert tex[1, 0].tolist() == list(texture_pixel(dl, [va] * 4, [0, 1, 2, 3]))  # row max_x - (-1)
    assert slice_pose[0] == 0.0
    img, ox, oy, _ = run_model(model, "image", proto, IDENTITY, tmp_path)
    assert img.shape == (1, 2)
    assert img.tolist() == [[image_byte([va] * 4), image_byte([vb, vb])]]
    assert (ox, oy) == (-1 * float(f32(0.1)), 0.0)


def test_model_image_wraps_modulo_256(dl, model, tmp_path):
    """Empty pixels are RoundToInt(-0.1 * 318.75) = -32 -> 224; a column's sum above ~0.9 wraps past 255."""
    v = int(dl.load_library().dliom_probability_to_value(C.c_float(0.9)))
    cells = [(0, 0, z, v) for z in range(3)] + [(1, 1, 0, v)]
    img, _, _, _ = run_model(model, "image", grid_proto(0.1, cells), IDENTITY, tmp_path)
    assert img.shape == (2, 2)
    assert img[0, 1] == 224 and img[1, 0] == 224
    assert img[1, 1] == image_byte([v]) == 255
    raw = lround(f32(f32(f32(f32(v2p(v) + v2p(v)) + v2p(v)) - P_MIN) * f32(f32(255) / (P_MAX - P_MIN))))
    assert raw > 255 and img[0, 0] == raw % 256


def test_model_empty_projections(dl, model, tmp_path):
    low = int(dl.load_library().dliom_probability_to_value(C.c_float(0.5)))
    for cells in ([], [(0, 0, 0, low), (1, 0, 0, low)]):
        proto = grid_proto(0.1, cells)
        assert run_model(model, "texture", proto, IDENTITY, tmp_path)[:2] == (0, 0)
        img, ox, oy, _ = run_model(model, "image", proto, IDENTITY, tmp_path)
        assert img.shape == (0, 0) and (ox, oy) == (0.0, 0.0)
