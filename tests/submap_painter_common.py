"""The CPU model of dliom.h "painting submap slices into one map" and the scenes its tests share.

The matrices are Python floats (IEEE doubles, one rounding an operation, in the statement's order); the pixels are
vectorised numpy on int64, no Python big integers, so a 300 x 300 map takes milliseconds.  A slice here is a dict
{cells (h, w, 2) uint8: intensity, alpha; resolution; slice_pose (7,); pose (7,)}."""
import ctypes as C
import ctypes.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARGUMENT, ERR_CAPACITY, ERR_TOO_LARGE = 0, -1, -9, -14
XRAY_MAX_PIXELS = 1 << 26
TILE = 16
BACKGROUND = 0xFF800000
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


# ---- Matrices (host_math.h's Rigid3d product, Eigen's SSE2 order) ---------------------------------------------------------
def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    t1x, t1y = aw * bx + ay * bz, aw * by + ay * bw
    t2x, t2y = az * bx - ax * bz, az * by - ax * bw
    u1z, u1w = aw * bz - ay * bx, aw * bw - ay * by
    u2z, u2w = az * bz + ax * bx, az * bw + ax * by
    return [u1w - u2z, t1x - t2y, t1y + t2x, u1z + u2w]


def _qnormalize(q):
    w, x, y, z = q
    z2 = (x * x + z * z) + (y * y + w * w)
    if z2 > 0.0:
        n = math.sqrt(z2)
        return [w / n, x / n, y / n, z / n]
    return q


def _qrot(q, v):
    uv = [q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]]
    uv = [u + u for u in uv]
    c = [q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]]
    return [(v[i] + q[0] * uv[i]) + c[i] for i in range(3)]


def pose_mul(a, b):
    a, b = [float(v) for v in a], [float(v) for v in b]
    rt = _qrot(a[3:], b[:3])
    return [rt[i] + a[i] for i in range(3)] + _qnormalize(_qmul(a[3:], b[3:]))


def cairo_matrix(s):
    """m = (xx, yx, xy, yy, x0, y0) of cairo_matrix_init(homo(1,0), homo(0,0), -homo(1,1), -homo(0,1), homo(0,3), -homo(1,3))"""
    P = pose_mul(s["pose"], s["slice_pose"])
    w, x, y, z = P[3:]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    r00, r01, r10, r11 = 1.0 - (ty * y + tz * z), ty * x - tz * w, ty * x + tz * w, 1.0 - (tx * x + tz * z)
    return (r10, r00, -r11, -r01, P[0], -P[1])


def slice_matrix(s, resolution):
    """L = (xx, yx, xy, yy, x0, y0)"""
    xx, yx, xy, yy, x0, y0 = cairo_matrix(s)
    k, sr = 1.0 / float(resolution), float(s["resolution"])
    return ((xx * k) * sr, (yx * k) * sr, (xy * k) * sr, (yy * k) * sr, x0 * k, y0 * k)


def _apply(m, x, y):
    xx, yx, xy, yy, x0, y0 = m
    return (xx * x + xy * y) + x0, (yx * x + yy * y) + y0


# ---- Layout, Inverse, Bound -----------------------------------------------------------------------------------------------
def layout(slices, resolution):
    """-> (status, width, height, origin float32[2], fixed int64 (n, 6): A B E C D G, matrices)"""
    f32 = np.float32
    mats = [slice_matrix(s, resolution) for s in slices]
    pts = []
    for s, m in zip(slices, mats):
        h, w = s["cells"].shape[:2]
        pts += [_apply(m, cx, cy) for cx, cy in ((0.0, 0.0), (float(w), 0.0), (0.0, float(h)), (float(w), float(h)))]
    pts = np.array(pts, np.float64).astype(f32)
    origin, size = np.zeros(2, f32), [0, 0]
    if not np.isfinite(pts).all():
        return ERR_TOO_LARGE, 0, 0, origin, None, mats
    for a in range(2):
        lo, hi = pts[:, a].min(), pts[:, a].max()
        extent = np.ceil(f32(hi - lo))
        if not extent < f32(2147483000.0):
            return ERR_TOO_LARGE, 0, 0, origin, None, mats
        size[a] = int(extent) + 10
        origin[a] = f32(-lo) + f32(5)
    if size[0] * size[1] > XRAY_MAX_PIXELS:
        return ERR_CAPACITY, size[0], size[1], origin, None, mats
    fixed = np.zeros((len(slices), 6), np.int64)
    for i, m in enumerate(mats):
        xx, yx, xy, yy = m[:4]
        x0, y0 = m[4] + float(origin[0]), m[5] + float(origin[1])
        det = xx * yy - yx * xy
        if det == 0.0:
            return ERR_TOO_LARGE, size[0], size[1], origin, None, mats
        inv = [yy / det, -xy / det, (xy * y0 - yy * x0) / det, -yx / det, xx / det, (yx * x0 - xx * y0) / det]
        if not all(math.isfinite(v) for v in inv):
            return ERR_TOO_LARGE, size[0], size[1], origin, None, mats
        for r in range(2):
            a, b, e = abs(inv[3 * r]), abs(inv[3 * r + 1]), abs(inv[3 * r + 2])
            if not a <= 1024.0 or not b <= 1024.0 or not a * size[0] + b * size[1] + e + 1.0 < 536870912.0:
                return ERR_TOO_LARGE, size[0], size[1], origin, None, mats
        fixed[i] = [int(np.rint(v * 4294967296.0)) for v in inv]
    return OK, size[0], size[1], origin, fixed, mats


# ---- Sample, Composite ----------------------------------------------------------------------------------------------------
def texels(cells):
    """(h, w, 4) int64: alpha, red, green, blue of alpha << 24 | intensity << 16 | observed << 8"""
    i, a = cells[..., 0].astype(np.int64), cells[..., 1].astype(np.int64)
    return np.stack([a, i, np.where((i == 0) & (a == 0), 0, 255), np.zeros_like(i)], axis=-1)


def _fetch(tex, x, y):
    h, w = tex.shape[:2]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(inside[..., None], tex[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)


def sample(tex, fixed, width, height, window=None):
    """the slice's bilinear sample at every pixel: (height, width, 4) int64; window (x0, y0, x1, y1): at those pixels only"""
    A, B, E, C, D, G = (np.int64(v) for v in fixed)
    left, top, right, bottom = window if window is not None else (0, 0, width - 1, height - 1)
    y, x = np.meshgrid(np.arange(top, bottom + 1, dtype=np.int64), np.arange(left, right + 1, dtype=np.int64), indexing="ij")
    half = np.int64(1) << np.int64(31)
    U = A * x + B * y + E + ((A + B) >> np.int64(1)) - half
    V = C * x + D * y + G + ((C + D) >> np.int64(1)) - half
    x1, y1 = U >> 32, V >> 32
    dx, dy = ((U >> 25) & 127) << 1, ((V >> 25) & 127) << 1
    w_br = dx * dy
    w_tr, w_bl = (dx << 8) - w_br, (dy << 8) - w_br
    w_tl = 65536 - (dx << 8) - (dy << 8) + w_br
    return (_fetch(tex, x1, y1) * w_tl[..., None] + _fetch(tex, x1 + 1, y1) * w_tr[..., None] +
            _fetch(tex, x1, y1 + 1) * w_bl[..., None] + _fetch(tex, x1 + 1, y1 + 1) * w_br[..., None]) >> 16


def mul8(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def composite(d, s):
    return np.minimum(255, s + mul8(d, 255 - s[..., :1]))


def pack(d):
    return (d[..., 0] << 24 | d[..., 1] << 16 | d[..., 2] << 8 | d[..., 3]).astype(np.uint32)


def paint(slices, resolution, windowed=False):
    """-> (status, pixels (height, width) uint32 or None, origin float32[2], width, height).  windowed: every slice is
    sampled inside its reach only (what the device's tile lists do) -- the same pixels, for maps too large to sample whole."""
    status, width, height, origin, fixed, mats = layout(slices, resolution)
    if status != OK:
        return status, None, origin, width, height
    d = np.zeros((height, width, 4), np.int64)
    d[..., 0], d[..., 1] = 255, 128
    for s, f, m in zip(slices, fixed, mats):
        h, w = s["cells"].shape[:2]
        if h == 0 or w == 0:
            continue
        if windowed:
            box = reach(m, origin, w, h, width, height)
            if box is not None:
                x0, y0, x1, y1 = box
                d[y0:y1 + 1, x0:x1 + 1] = composite(d[y0:y1 + 1, x0:x1 + 1], sample(texels(s["cells"]), f, width, height, box))
        else:
            d = composite(d, sample(texels(s["cells"]), f, width, height))
    return OK, pack(d), origin, width, height


# ---- Grid -----------------------------------------------------------------------------------------------------------------
def occupancy_table():
    out = np.zeros(256, np.int8)
    for c in range(256):
        v = (1.0 - c / 255.0) * 100.0
        t = math.floor(v)
        out[c] = t + (1 if v - t >= 0.5 else 0)  # lround of a value >= 0
    return out


def occupancy(pixels, origin, resolution):
    """-> (data (height, width) int8, origin_xy float64[2])"""
    flipped = pixels[::-1]
    red, green = (flipped >> 16) & 255, (flipped >> 8) & 255
    data = np.where(green == 0, np.int8(-1), occupancy_table()[red]).astype(np.int8)
    height = pixels.shape[0]
    origin_xy = np.array([float(-origin[0]) * float(resolution),
                          float(np.float32(-height) + np.float32(origin[1])) * float(resolution)], np.float64)
    return data, origin_xy


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def yaw_pose(x, y, yaw, z=0.0):
    return np.array([x, y, z, math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw)], np.float64)


def random_pose(rng, reach, tilt=0.2):
    """a pose within +-reach metres, any yaw, roll and pitch within +-tilt rad"""
    roll, pitch, yaw = rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-math.pi, math.pi)
    cr, sr, cp, sp, cy, sy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (math.cos, math.sin))
    q = [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]
    return np.array(list(rng.uniform(-reach, reach, 3)) + q, np.float64)


def random_cells(rng, h, w, alpha="random"):
    """(h, w, 2) uint8 like an X-ray texture's: a third of the texels never observed (0, 0); alpha: 'random', 0 or 255"""
    cells = rng.integers(0, 256, (h, w, 2)).astype(np.uint8)
    if alpha != "random":
        cells[..., 1] = alpha
    cells[rng.random((h, w)) < 1.0 / 3.0] = 0
    return cells


def make_slice(cells, resolution, pose, slice_pose=IDENTITY):
    return dict(cells=np.ascontiguousarray(cells, np.uint8), resolution=float(resolution),
                slice_pose=np.asarray(slice_pose, np.float64), pose=np.asarray(pose, np.float64))


def random_layout(seed):
    """1-5 slices (zero-size ones included), resolutions 0.05 / 0.10 / 0.45, poses within +-500 m -> (slices, resolution)"""
    rng = np.random.default_rng(seed)
    centre = random_pose(rng, 500.0)
    slices = []
    for _ in range(int(rng.integers(1, 6))):
        h, w = (0, 0) if rng.random() < 0.15 else (int(rng.integers(0, 40)), int(rng.integers(0, 40)))
        pose = random_pose(rng, 500.0)
        pose[:3] = centre[:3] + rng.uniform(-8.0, 8.0, 3)  # a map of a few hundred pixels, wherever it lies
        slices.append(make_slice(np.zeros((h, w, 2), np.uint8), rng.choice([0.05, 0.10, 0.45]), pose, random_pose(rng, 3.0, 0.05)))
    return slices, float(rng.choice([0.03, 0.05, 0.10]))


def describe(dl, s):
    return dl.submap_slice_description(s["cells"].shape[1], s["cells"].shape[0], s["resolution"], s["slice_pose"], s["pose"])


# ---- the system's cairo, where there is one -------------------------------------------------------------------------------
class _CairoMatrix(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("xx", "yx", "xy", "yy", "x0", "y0")]


def load_cairo():
    """libcairo through ctypes, or None"""
    name = ctypes.util.find_library("cairo")
    if name is None:
        return None
    try:
        lib = C.CDLL(name)
    except OSError:
        return None
    vp, d = C.c_void_p, C.c_double
    for fn, res, args in (("cairo_image_surface_create", vp, [C.c_int, C.c_int, C.c_int]),
                          ("cairo_image_surface_create_for_data", vp, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
                          ("cairo_format_stride_for_width", C.c_int, [C.c_int, C.c_int]),
                          ("cairo_create", vp, [vp]), ("cairo_destroy", None, [vp]), ("cairo_surface_destroy", None, [vp]),
                          ("cairo_scale", None, [vp, d, d]), ("cairo_translate", None, [vp, d, d]),
                          ("cairo_save", None, [vp]), ("cairo_restore", None, [vp]),
                          ("cairo_transform", None, [vp, C.POINTER(_CairoMatrix)]),
                          ("cairo_user_to_device", None, [vp, C.POINTER(d), C.POINTER(d)]),
                          ("cairo_set_source_rgba", None, [vp, d, d, d, d]), ("cairo_paint", None, [vp]),
                          ("cairo_set_source_surface", None, [vp, vp, d, d]), ("cairo_surface_flush", None, [vp]),
                          ("cairo_surface_status", C.c_int, [vp]), ("cairo_status", C.c_int, [vp]),
                          ("cairo_get_source", vp, [vp]), ("cairo_pattern_set_filter", None, [vp, C.c_int]),
                          ("cairo_image_surface_get_data", vp, [vp]), ("cairo_image_surface_get_stride", C.c_int, [vp]),
                          ("cairo_version_string", C.c_char_p, [])):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args
    return lib


CAIRO_FILTER_BILINEAR = 4


def cairo_paint(lib, slices, resolution, pattern_filter=None):
    """io::PaintSubmapSlices' own call sequence (submap_painter.cc:30-108, DrawTexture :158-185) on the system's cairo ->
    (pixels (height, width) uint32, origin float32[2]).  pattern_filter: None leaves cairo's default (CAIRO_FILTER_GOOD),
    as the reference does."""
    f32, ARGB32 = np.float32, 0

    def walk(cr, callback):  # CairoPaintSubmapSlices
        lib.cairo_scale(cr, 1.0 / resolution, 1.0 / resolution)
        for s in slices:
            lib.cairo_save(cr)
            m = _CairoMatrix(*cairo_matrix(s))
            lib.cairo_transform(cr, C.byref(m))
            lib.cairo_scale(cr, s["resolution"], s["resolution"])
            callback(s)
            lib.cairo_restore(cr)

    surface = lib.cairo_image_surface_create(ARGB32, 1, 1)
    cr = lib.cairo_create(surface)
    points = []

    def corners(s):
        h, w = s["cells"].shape[:2]
        for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
            px, py = C.c_double(x), C.c_double(y)
            lib.cairo_user_to_device(cr, C.byref(px), C.byref(py))
            points.append((px.value, py.value))

    walk(cr, corners)
    lib.cairo_destroy(cr)
    lib.cairo_surface_destroy(surface)
    p = np.array(points, np.float64).astype(f32)  # Eigen::AlignedBox2f::extend(Vector2f(x, y))
    lo, hi = p.min(axis=0), p.max(axis=0)
    width, height = (int(np.ceil(f32(hi[a] - lo[a])) + f32(10)) for a in range(2))
    origin = (-lo + f32(5)).astype(f32)

    textures = []
    for s in slices:  # DrawTexture
        i, a = s["cells"][..., 0].astype(np.uint32), s["cells"][..., 1].astype(np.uint32)
        observed = np.where((i == 0) & (a == 0), 0, 255).astype(np.uint32)
        data = np.ascontiguousarray(a << 24 | i << 16 | observed << 8)
        h, w = data.shape
        assert lib.cairo_format_stride_for_width(ARGB32, w) == 4 * w
        surf = lib.cairo_image_surface_create_for_data(data.ctypes.data, ARGB32, w, h, 4 * w)
        assert lib.cairo_surface_status(surf) == 0
        textures.append((data, surf))
    surface = lib.cairo_image_surface_create(ARGB32, width, height)
    cr = lib.cairo_create(surface)
    lib.cairo_set_source_rgba(cr, 0.5, 0.0, 0.0, 1.0)
    lib.cairo_paint(cr)
    lib.cairo_translate(cr, float(origin[0]), float(origin[1]))
    order = iter(textures)

    def draw(s):
        lib.cairo_set_source_surface(cr, next(order)[1], 0.0, 0.0)
        if pattern_filter is not None:
            lib.cairo_pattern_set_filter(lib.cairo_get_source(cr), pattern_filter)
        lib.cairo_paint(cr)

    walk(cr, draw)
    lib.cairo_surface_flush(surface)
    assert lib.cairo_status(cr) == 0
    stride = lib.cairo_image_surface_get_stride(surface)
    raw = C.string_at(lib.cairo_image_surface_get_data(surface), stride * height)
    pixels = np.frombuffer(raw, np.uint8).reshape(height, stride)[:, :4 * width].copy().view(np.uint32).reshape(height, width)
    lib.cairo_destroy(cr)
    lib.cairo_surface_destroy(surface)
    for _, surf in textures:
        lib.cairo_surface_destroy(surf)
    return pixels, origin


def channel_differences(a, b):
    """largest absolute difference per channel (alpha, red, green, blue) of two ARGB images, and the share of equal pixels"""
    d = [int(np.abs(((a >> sh) & 255).astype(np.int64) - ((b >> sh) & 255).astype(np.int64)).max()) for sh in (24, 16, 8, 0)]
    return d, float((a == b).mean())


def cairo_scenes():
    """the fixed list the statement is checked on against cairo: (name, slices, resolution), all resolution <= the slices'"""
    rng = np.random.default_rng(2024)
    scenes = []
    for k, (res, sr, yaw) in enumerate([(0.05, 0.10, 0.3), (0.05, 0.10, -1.2), (0.10, 0.10, 0.5), (0.05, 0.45, 2.0),
                                        (0.10, 0.45, -0.4), (0.03, 0.05, 0.9)]):
        n = 12 if sr == 0.45 else 40
        a = make_slice(random_cells(rng, n, n + 7), sr, yaw_pose(1.0 * k, -2.0 * k, yaw), yaw_pose(0.3, -0.2, 0.0, 0.5))
        b = make_slice(random_cells(rng, n + 5, n), sr, random_pose(rng, 1.5, 0.1), random_pose(rng, 0.5, 0.02))
        b["pose"][:2] += a["pose"][:2]
        scenes.append(("two slices %d" % k, [a, b], res))
    aligned = make_slice(random_cells(rng, 30, 45), 0.10, IDENTITY)
    scenes.append(("axis-aligned, equal resolution", [aligned], 0.10))
    far = []
    for k in range(4):
        pose = random_pose(rng, 2.0, 0.05)
        pose[:2] += (300.0, -300.0)
        far.append(make_slice(random_cells(rng, 90, 110), 0.10, pose, random_pose(rng, 1.0, 0.02)))
    scenes.append(("300 m from the origin", far, 0.05))
    return scenes


def coarse_scene():
    """a map 2x coarser than its slice: cairo's GOOD filter is a box convolution there, the statement stays bilinear"""
    rng = np.random.default_rng(77)
    return [make_slice(random_cells(rng, 60, 60), 0.05, yaw_pose(0.5, 0.5, 0.4))], 0.10


# ---- the tile lists' sizing (submap_painter_layout.h: reach, tile_pairs) ---------------------------------------------------
def reach(m, origin, w, h, width, height):
    """the pixel box [x0, x1] x [y0, y1] a slice's list entries come from, or None"""
    if w == 0 or h == 0:
        return None
    F = m[:4] + (m[4] + float(origin[0]), m[5] + float(origin[1]))
    p = np.array([_apply(F, cx, cy) for cx, cy in ((-1.0, -1.0), (w + 1.0, -1.0), (-1.0, h + 1.0), (w + 1.0, h + 1.0))])
    lo, hi = np.floor(p.min(axis=0)) - 1.0, np.ceil(p.max(axis=0)) + 1.0
    x0, y0 = (int(min(max(lo[a], 0.0), (width, height)[a])) for a in range(2))
    x1, y1 = (int(max(min(hi[a], (width, height)[a] - 1.0), -1.0)) for a in range(2))
    return None if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)


def tile_pairs(slices, resolution):
    status, width, height, origin, _, mats = layout(slices, resolution)
    assert status == OK
    pairs = 0
    for s, m in zip(slices, mats):
        b = reach(m, origin, s["cells"].shape[1], s["cells"].shape[0], width, height)
        if b is not None:
            pairs += (b[2] // TILE - b[0] // TILE + 1) * (b[3] // TILE - b[1] // TILE + 1)
    return pairs
