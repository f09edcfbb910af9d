"""Submap image features (dliom.h "submap image features") without a GPU: the CPU model (tests/cpp/surf_model.cc) against
independent code -- scipy's minimum filter, numpy's cumsum, a numpy float32 restatement of the layers, atan2 -- and
against what SURF is for: a disc is found where it is, and an image and its rotated, shifted copy match.  OpenCV cannot
pin the statement (it is not a dependency), so this is where its worth is shown."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_match_common as fm
import surf_common as sc


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("surf_model")
    return sc.build_model(d), d


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.mark.parametrize("k", sc.ERODE_KS)
def test_binarize_erode_equals_scipy(model, k):
    """Step 1 against scipy.ndimage.minimum_filter of the numpy threshold: pixels outside take no part (cval = 255 among
    {0, 255}), and anchor (k / 2, k / 2) is scipy's origin 0 (its window of size k starts at -(k // 2))."""
    from scipy import ndimage
    exe, d = model
    for H, W, seed in sc.ERODE_SHAPES:
        img = sc.random_bytes(H, W, seed)
        for threshold in (200, 0, 255):
            binary = np.where(img > threshold, 255, 0).astype(np.uint8)
            want = ndimage.minimum_filter(binary, size=k, mode="constant", cval=255, origin=0)
            assert np.array_equal(sc.model_binarize_erode(exe, d, img, threshold, k), want), (H, W, threshold)


def test_integral_equals_cumsum(model):
    exe, d = model
    for H, W, seed in sc.ERODE_SHAPES:
        img = sc.random_bytes(H, W, seed)
        want = np.zeros((H + 1, W + 1), np.int64)
        want[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
        assert np.array_equal(sc.model_integral(exe, d, img), want)


TEMPLATES = {"dxx": [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)], "dyy": [(2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1)],
             "dxy": [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]}


def numpy_layer(img, octave, layer):
    """Step 3 in numpy float32: whole-array operations, each one rounded to float32 on its own."""
    f = np.float32
    H, W = img.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    size, step = (9 + 6 * layer) << octave, 1 << octave
    rows, cols = H // step, W // step
    det, trace = np.zeros((rows, cols), f), np.zeros((rows, cols), f)
    if size > H or size > W:
        return det, trace
    ni, nj, m = 1 + (H - size) // step, 1 + (W - size) // step, (size // 2) // step
    ys, xs = (np.arange(ni) * step)[:, None], (np.arange(nj) * step)[None, :]
    ratio = f(size) / f(9)
    resp = {}
    for name, boxes in TEMPLATES.items():
        r = np.zeros((ni, nj), f)
        for box in boxes:
            x1, y1, x2, y2 = (int(np.rint(ratio * f(c))) for c in box[:4])
            w = f(box[4]) / f((x2 - x1) * (y2 - y1))
            total = S[ys + y1, xs + x1] + S[ys + y2, xs + x2] - S[ys + y2, xs + x1] - S[ys + y1, xs + x2]
            r = r + total.astype(f) * w
        resp[name] = r
    det[m:m + ni, m:m + nj] = resp["dxx"] * resp["dyy"] - (f(0.81) * resp["dxy"]) * resp["dxy"]
    trace[m:m + ni, m:m + nj] = resp["dxx"] + resp["dyy"]
    return det, trace


def test_templates_equal_header():
    header = open(os.path.join(sc.ROOT, "include", "dliom.h")).read()
    for name, boxes in TEMPLATES.items():
        text = re.search(r"#define DLIOM_SURF_TEMPLATE_%s (.*)" % name.upper(), header).group(1)
        assert eval(text.replace("{", "(").replace("}", ")")) == tuple(boxes)


@pytest.mark.parametrize("octave,layer", sc.LAYERS)
def test_layers_equal_numpy_float32(model, octave, layer):
    exe, d = model
    H, W, seed = sc.LAYER_IMAGE
    for img in (sc.random_bytes(H, W, seed), sc.blob_image(H, W, 12, seed=3)):
        det, trace = sc.model_layer(exe, d, img, octave, layer)
        want_det, want_trace = numpy_layer(img, octave, layer)
        assert det.shape == want_det.shape
        assert np.array_equal(det.view(np.uint32), want_det.view(np.uint32))
        assert np.array_equal(trace.view(np.uint32), want_trace.view(np.uint32))
    assert (det != 0).any() == ((9 + 6 * layer) << octave <= min(H, W))


def test_fast_atan2_within_a_fiftieth_of_a_degree(model):
    """10^5 directions at mixed magnitudes and the axes.  (Over 2 * 10^6 directions the polynomial's error is 0.0096 deg.)"""
    exe, d = model
    rng = np.random.RandomState(1)
    phi = rng.uniform(0, 2 * np.pi, 100000)
    r = np.exp(rng.uniform(-10, 10, phi.size))
    y, x = (r * np.sin(phi)).astype(np.float32), (r * np.cos(phi)).astype(np.float32)
    y[:4], x[:4] = [0, 1, 0, -1], [1, 0, -1, 0]
    got = sc.model_fast_atan2(exe, d, y, x).astype(np.float64)
    want = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0
    err = np.abs(got - want)
    err = np.minimum(err, 360.0 - err)
    print("fastAtan2 max error %.5f deg" % err.max())
    assert err.max() <= 0.02
    assert sc.model_fast_atan2(exe, d, [0.0], [0.0])[0] == 0.0


def test_disc_is_found_where_it_is(model):
    """A white disc on black: the strongest key point lies within one pixel of its centre, and a larger disc gets a
    larger size."""
    exe, d = model
    sizes = []
    for cx, cy, r in ((100, 90, 6), (83, 117, 11), (120, 101, 20)):
        status, n, kp, desc = sc.model_detect_and_compute(exe, d, sc.disc_image(200, 220, [(cx, cy, r)]), sc.Options(k=1))
        assert status == sc.OK and n >= 1
        assert abs(kp[0, 0] - cx) <= 1.0 and abs(kp[0, 1] - cy) <= 1.0, kp[0]
        assert kp[0, 6] == -1.0  # a bright blob: negative trace
        assert (np.diff(kp[:, 4]) <= 0).all()  # response descending
        assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-5)
        sizes.append(kp[0, 2])
    assert sizes[0] < sizes[1] < sizes[2], sizes


def test_covariance_end_to_end(model, tmp_path):
    """An image of 60 irregular blobs and the same image rotated by 90 degrees (an exact permutation) and shifted by whole
    pixels inside a larger canvas; the two feature sets through feature_match_model with pose_graph.lua's options at
    resolution 0.1: MATCHED, theta within 5 degrees of +-90, the canvas's centre mapped to within the RANSAC threshold of
    where the planted motion puts it, and at least twice minimum_good_match_num inliers."""
    exe, d = model
    fexe = fm.build_model(tmp_path)
    A, B, k, (sx, sy) = sc.covariance_scene()
    assert k == 1
    options = sc.Options()
    sa, na, kpa, da = sc.model_detect_and_compute(exe, d, A, options)
    sb, nb, kpb, db = sc.model_detect_and_compute(exe, d, B, options)
    assert sa == sb == sc.OK and na >= 50 and nb >= 50
    sets = [fm.FeatureSet(da, kpa[:, :2], 0.0, 0.0, 0.1), fm.FeatureSet(db, kpb[:, :2], 0.0, 0.0, 0.1)]
    match = fm.Options(ratio=0.5, minimum_good=5, threshold=3.0, tolerance=0.1, seed=7)
    r = fm.model_match(fexe, tmp_path, sets, 0, [1], match)[0][0]
    print("key points %d / %d, good matches %d, inliers %d, theta %.4f deg" % (na, nb, r["good_matches"], r["inliers"],
                                                                             np.degrees(r["theta"])))
    check_planted_motion(r, A.shape, (sx, sy), match)


def check_planted_motion(r, shape, shift, match, resolution=0.1):
    """A's pixel (x, y) lies at (y + sx, (W - 1 - x) + sy) in B (numpy.rot90 once)."""
    H, W = shape
    assert r["status"] == fm.MATCHED
    assert r["inliers"] >= 2 * match.minimum_good
    assert abs(abs(np.degrees(r["theta"])) - 90.0) <= 5.0
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    want = np.array([cy + shift[0], (W - 1 - cx) + shift[1]]) * resolution
    got = np.array([r["a"] * cx * resolution - r["b"] * cy * resolution + r["tx"],
                    r["b"] * cx * resolution + r["a"] * cy * resolution + r["ty"]])
    assert np.linalg.norm(got - want) <= match.threshold, (got, want)


def test_constants_and_symbols(dl):
    header = open(os.path.join(sc.ROOT, "include", "dliom.h")).read()
    assert int(re.search(r"#define DLIOM_SURF_MAX_KEYPOINTS (\d+)", header).group(1)) == sc.MAX_KEYPOINTS == dl.SURF_MAX_KEYPOINTS
    assert int(re.search(r"#define DLIOM_SURF_MAX_STRUCTURE_ELEMENT (\d+)", header).group(1)) == dl.SURF_MAX_STRUCTURE_ELEMENT
    assert "#define DLIOM_SURF_MAX_PIXELS (1 << 23)" in header and dl.SURF_MAX_PIXELS == 1 << 23
    assert int(re.search(r"#define DLIOM_SURF_ORI_SAMPLES (\d+)", header).group(1)) == \
        sum(1 for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36)
    names = {n for n, _, _ in dl.SYMBOLS}
    L = dl.load_library()
    for n in ("dliom_surf_default_options", "dliom_image_binarize_erode", "dliom_surf_layer", "dliom_surf_detect_and_compute",
              "dliom_feature_index_add_from_grid"):
        assert n in names and getattr(L, n) is not None
    assert header.lower().count("parity unpinned against opencv") >= 2
    o = L.dliom_surf_default_options()
    assert (o.binary_threshold, o.structure_element_size, o.hessian_threshold, o.n_octaves, o.n_octave_layers, o.extended,
            o.upright) == (200, 3, 400.0, 4, 3, 0, 0)
    p = dl.surf_options()
    assert bytes(p) == bytes(o)


def test_struct_layout_matches_header(dl, tmp_path):
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dliom.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(dliom_surf_options), offsetof(dliom_surf_options, hessian_threshold), '
                   'offsetof(dliom_surf_options, upright)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(sc.ROOT, "include"), "-o", str(exe), str(src)])
    size, hessian, upright = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(dl.SurfOptions) and hessian == dl.SurfOptions.hessian_threshold.offset
    assert upright == dl.SurfOptions.upright.offset


def test_argument_checks_without_a_context(dl):
    """Every new entry point refuses a NULL context, index or grid before it touches the device.  (The refused options
    need a context to be told apart from that: tests/test_gpu_surf.py::test_refused_options.)"""
    L = dl.load_library()
    o = dl.surf_options()
    img = np.zeros((8, 8), np.uint8)
    out = np.zeros((8, 8), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    n, rows, cols = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.dliom_image_binarize_erode(None, img.ctypes.data_as(u8), 8, 8, C.byref(o), out.ctypes.data_as(u8)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_surf_layer(None, img.ctypes.data_as(u8), 8, 8, 0, 0, None, None, C.byref(rows), C.byref(cols)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_surf_detect_and_compute(None, img.ctypes.data_as(u8), 8, 8, C.byref(o), None, None, 0, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
    pose = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    assert L.dliom_feature_index_add_from_grid(None, 1, None, pose, C.byref(o), C.byref(n), None, None, None) == dl.ERR_INVALID_ARGUMENT


def test_adapter_compiles(dl, tmp_path):
    """tests/cpp/surf_adapter.cc (SubmapFeatureMatcher::AddSubmap from a HybridGrid) builds with plain g++."""
    import subprocess
    libdir = os.path.join(sc.ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(sc.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", str(tmp_path / "surf_adapter"),
                           os.path.join(sc.ROOT, "tests", "cpp", "surf_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
