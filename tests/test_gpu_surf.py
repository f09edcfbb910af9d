"""Submap image features on the device (dliom.h "submap image features") against the CPU model
(tests/cpp/surf_model.cc): every byte equal -- eroded images, det / trace arrays, key point records and descriptors.  No
tolerances: the statement has no order freedom.

The wavelet-size rule of step 6 (H + 1 < side) cannot fire behind step 4: a kept candidate of layer l needs
H > size_{l+1} >= its refined size, and side = 2 round(2.4 size / 9) < 0.54 size + 1.  The case `largest_in_small_image`
holds the largest sizes an image admits; the rule itself is shared code with the model and stays in both."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import feature_match_common as fm
import surf_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("surf_model")
    return sc.build_model(d), d


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_binarize_erode_equals_model(dl, ctx, model, k):
    exe, d = model
    for H, W, seed in sc.ERODE_SHAPES:
        img = sc.random_bytes(H, W, seed)
        for threshold in (200, 0, 255):
            got = dl.image_binarize_erode(ctx, img, dl.surf_options(threshold, k))
            assert np.array_equal(got, sc.model_binarize_erode(exe, d, img, threshold, k)), (H, W, threshold)


def test_layers_equal_model(dl, ctx, model):
    """Every (octave, layer) of a 97 x 130 image of random bytes (those that do not fit included: zeros of the right
    size) and octave 3 of a 300 x 280 one."""
    exe, d = model
    H, W, seed = sc.LAYER_IMAGE
    img = sc.random_bytes(H, W, seed)
    for octave, layer in sc.LAYERS:
        det, trace = dl.surf_layer(ctx, img, octave, layer)
        want_det, want_trace = sc.model_layer(exe, d, img, octave, layer)
        assert same_bits(det, want_det) and same_bits(trace, want_trace), (octave, layer)
    big = sc.random_bytes(280, 300, 7)
    for layer in (0, 4):
        det, trace = dl.surf_layer(ctx, big, 3, layer)
        want_det, want_trace = sc.model_layer(exe, d, big, 3, layer)
        assert same_bits(det, want_det) and same_bits(trace, want_trace) and (det != 0).any()


def leaves_image(kp, W, H):
    """Per border of a W x H image: does some key point have an orientation sample that step 6 skips there (the wavelet
    at the offset of -6 or +6 leaves the integral image) and a descriptor window that step 7 clamps there (the rotated
    window reaches at least (w - 1) / 2 from its centre in every direction)?  The statement's own float arithmetic."""
    f = np.float32
    found = dict(left=False, right=False, top=False, bottom=False)
    for x, y, size in kp[:, :3]:
        s = f(size) * f(1.2) / f(9.0)
        side = 2 * int(np.rint(f(2.0) * s))
        half = f(side - 1) / f(2.0)
        reach = (int(f(21.0) * s) - 1) / 2.0
        low = lambda c: int(np.rint((c + f(-6) * s) - half)) < 0 and c - reach < -0.5
        high = lambda c, n: int(np.rint((c + f(6) * s) - half)) >= n + 1 - side and c + reach > n - 0.5
        found["left"] |= bool(low(x))
        found["top"] |= bool(low(y))
        found["right"] |= bool(high(x, W))
        found["bottom"] |= bool(high(y, H))
    return found


EXPECTED = {"8x8_no_layer": lambda kp: len(kp) == 0, "40x37_octave0": lambda kp: len(kp) == 1 and kp[0, 5] == 0,
            "97x130_two_octaves": lambda kp: set(kp[:, 5]) == {0.0, 1.0}, "300x280_four_octaves": lambda kp: set(kp[:, 5]) == {0.0, 1.0, 2.0, 3.0},
            "one_keypoint": lambda kp: len(kp) == 1, "all_white": lambda kp: len(kp) == 0, "all_black": lambda kp: len(kp) == 0,
            "borders": lambda kp: len(kp) >= 5 and all(leaves_image(kp, 110, 90).values()),
            "largest_in_small_image": lambda kp: kp[:, 2].max() > 100, "one_octave": lambda kp: set(kp[:, 5]) == {0.0}}


@pytest.mark.parametrize("name", sorted(sc.DETECT_CASES))
def test_detect_and_compute_equals_model(dl, ctx, model, name):
    exe, d = model
    img, options = sc.DETECT_CASES[name]
    status, count, want_kp, want_desc = sc.model_detect_and_compute(exe, d, img, options)
    assert status == sc.OK
    kp, desc = dl.surf_detect_and_compute(ctx, img, options.device(dl))
    print(name, "key points: device %d, model %d" % (len(kp), count))
    assert len(kp) == count
    assert same_bits(kp, want_kp)
    assert same_bits(desc, want_desc)
    if name in EXPECTED:
        assert EXPECTED[name](want_kp), want_kp[:8]
    again_kp, again_desc = dl.surf_detect_and_compute(ctx, img, options.device(dl))
    assert same_bits(again_kp, kp) and same_bits(again_desc, desc)


def test_scratch_grown_after_a_call_without_candidates(dl, model):
    """A fresh context whose first call finds no candidate (a black image: only the image-sized scratch exists, so the
    allocation that replaces it may start where it did), then images that make that scratch grow: the Gaussian tables and
    the orientation offsets live in it and must be there again after every growth."""
    exe, d = model
    c = dl.Context(0)
    try:
        for name in ("all_black", "97x130_two_octaves", "all_black", "300x280_blobs", "97x130_two_octaves"):
            img, options = sc.DETECT_CASES[name]
            _, _, want_kp, want_desc = sc.model_detect_and_compute(exe, d, img, options)
            kp, desc = dl.surf_detect_and_compute(c, img, options.device(dl))
            assert same_bits(kp, want_kp) and same_bits(desc, want_desc), name
    finally:
        c.close()


def test_capacity_one_too_small(dl, ctx):
    img, options = sc.DETECT_CASES["97x130_two_octaves"]
    L, o = dl.load_library(), options.device(dl)
    u8, f32 = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    img = np.ascontiguousarray(img)
    n = C.c_int32()
    args = (ctx.h, img.ctypes.data_as(u8), img.shape[1], img.shape[0], C.byref(o))
    assert L.dliom_surf_detect_and_compute(*args, None, None, 0, C.byref(n)) == dl.OK
    count = n.value
    assert count > 1
    kp, desc = np.full((count, 7), -7, np.float32), np.full((count, 64), -7, np.float32)
    n.value = 0
    assert L.dliom_surf_detect_and_compute(*args, kp.ctypes.data_as(f32), desc.ctypes.data_as(f32), count - 1,
                                           C.byref(n)) == dl.ERR_CAPACITY
    assert n.value == count and (kp == -7).all() and (desc == -7).all()
    assert L.dliom_surf_detect_and_compute(*args, kp.ctypes.data_as(f32), desc.ctypes.data_as(f32), count, C.byref(n)) == dl.OK
    assert n.value == count and (kp[:, 4] > 400).all()


def test_more_candidates_than_the_capacity(dl, ctx, model):
    """More than DLIOM_SURF_MAX_KEYPOINTS candidates: DLIOM_ERR_CAPACITY whatever the buffers, with the model's count of
    them (the candidates beyond the capacity take no slot); the context works afterwards."""
    exe, d = model
    img, options = sc.over_capacity_case()
    status, candidates, _, _ = sc.model_detect_and_compute(exe, d, img, options)
    assert status == sc.ERR_CAPACITY and candidates > sc.MAX_KEYPOINTS
    L, o = dl.load_library(), options.device(dl)
    n = C.c_int32()
    assert L.dliom_surf_detect_and_compute(ctx.h, img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0], C.byref(o),
                                           None, None, 0, C.byref(n)) == dl.ERR_CAPACITY
    assert n.value == candidates
    small, small_options = sc.DETECT_CASES["40x37_octave0"]
    assert len(dl.surf_detect_and_compute(ctx, small, small_options.device(dl))[0]) == 1


def test_refused_options(dl, ctx):
    img = sc.DETECT_CASES["40x37_octave0"][0]
    assert len(dl.surf_detect_and_compute(ctx, img, dl.surf_options(structure_element_size=1))[0]) == 1
    bad = [dict(extended=1), dict(upright=1), dict(n_octaves=0), dict(n_octaves=5), dict(n_octave_layers=0),
           dict(n_octave_layers=4), dict(hessian_threshold=-1.0), dict(hessian_threshold=float("nan")),
           dict(hessian_threshold=float("inf")), dict(structure_element_size=0),
           dict(structure_element_size=dl.SURF_MAX_STRUCTURE_ELEMENT + 1), dict(binary_threshold=-1), dict(binary_threshold=256)]
    for kw in bad:
        with pytest.raises(dl.DliomError) as e:
            dl.surf_detect_and_compute(ctx, img, dl.surf_options(**kw))
        assert e.value.status == dl.ERR_INVALID_ARGUMENT, kw
        with pytest.raises(dl.DliomError) as e:
            dl.image_binarize_erode(ctx, img, dl.surf_options(**kw))
        assert e.value.status == dl.ERR_INVALID_ARGUMENT, kw
    L = dl.load_library()
    n = C.c_int32()
    o = dl.surf_options()
    assert L.dliom_surf_detect_and_compute(ctx.h, None, 4096, 4096, C.byref(o), None, None, 0, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
    big = np.zeros(1, np.uint8)  # never read: the size is refused first
    assert L.dliom_surf_detect_and_compute(ctx.h, big.ctypes.data_as(C.POINTER(C.c_uint8)), 4096, 2049, C.byref(o), None, None, 0,
                                           C.byref(n)) == dl.ERR_TOO_LARGE


# ---- from a grid ---------------------------------------------------------------------------------------------------
IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def scene_grid(dl, ctx, quarter_turns=0, resolution=0.1, scans=6):
    """The synthetic scene's scans inserted at ground truth; quarter_turns: the world rotated about z by that many right
    angles first (an exact permutation of the points' coordinates)."""
    from dliom import synth
    ins = dl.RangeDataInserter3D(0.55, 0.49, 2, ctx=ctx)
    g = dl.HybridGrid(ctx, resolution)
    for s in range(scans):
        pose = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(pose, 16, 256)
        world = synth.transform_points(pose, pts).astype(np.float32)
        origin = pose[:3].astype(np.float32)
        for _ in range(quarter_turns % 4):
            world = np.stack([-world[:, 1], world[:, 0], world[:, 2]], axis=1)
            origin = np.array([-origin[1], origin[0], origin[2]], np.float32)
        ins.Insert(origin, np.ascontiguousarray(world), g)
    return g


def test_add_from_grid_equals_the_three_calls(dl, ctx, orc):
    """dliom_feature_index_add_from_grid against dliom_grid_project_to_image -> dliom_surf_detect_and_compute ->
    dliom_feature_index_add: the same count and corner, and through dliom_feature_index_knn every stored descriptor at
    distance 0 from its own copy, with the same second neighbour as the old route against itself."""
    from helpers import build_oracle_submap, to_device_grid
    g = to_device_grid(dl, ctx, build_oracle_submap(orc, 0.10, num_scans=6, beams=16, azimuths=256))
    options = dl.surf_options()
    image, ox, oy, resolution = dl.grid_project_to_image(g, IDENTITY)
    kp, desc = dl.surf_detect_and_compute(ctx, image, options)
    print("projection %s, key points %d" % (image.shape, len(kp)))
    assert len(kp) >= 2
    index = dl.FeatureIndex(ctx, 64)
    index.add(1, desc, kp[:, :2], ox, oy, resolution)
    assert index.add_from_grid(2, g, IDENTITY, options) == (len(kp), ox, oy, resolution)
    index.add(3, desc, kp[:, :2] + np.float32(0.5), ox, oy, resolution)  # other key points: seen by the match below
    j0, j1, d0, d1 = index.knn(2, 1, len(kp))
    k0, k1, e0, e1 = index.knn(1, 1, len(kp))
    assert (d0 == 0).all() and same_bits(j0, k0) and same_bits(j1, k1) and same_bits(d1, e1) and same_bits(d0, e0)
    # the stored key points: a match of the new set against the old one is the old one against itself, bit for bit
    match = dl.feature_match_options(0.9, 2, 3.0, 0.1, 7)
    new, _ = index.match(2, [1, 3], match)
    old, _ = index.match(1, [1, 3], match)
    assert new.tobytes() == old.tobytes() and new[0]["status"] == fm.MATCHED
    with pytest.raises(dl.DliomError):
        index.add_from_grid(2, g, IDENTITY, options)  # a duplicate key
    other = dl.FeatureIndex(ctx, 32)
    with pytest.raises(dl.DliomError):
        other.add_from_grid(1, g, IDENTITY, options)  # descriptor size 64 only
    other.close()
    empty = dl.HybridGrid(ctx, 0.1)
    assert index.add_from_grid(9, empty, IDENTITY, options)[0] == 0  # an empty projection: an empty set
    r, _ = index.match(9, [1], match)
    assert r[0]["status"] == fm.TOO_FEW_KEYPOINTS
    empty.close()
    index.close()
    g.close()


def test_yawed_grids_match(dl, ctx):
    """Two grids of one scene, one with the world turned by 90 degrees, each projected at the identity and stored with
    dliom_feature_index_add_from_grid; matched with pose_graph.lua's options: the host covariance test's bars (MATCHED,
    at least twice minimum_good_match_num inliers, theta within 5 degrees of +-90, the image centre within the RANSAC
    threshold of where the planted turn puts it: a world point (x, y) lies at (-y, x))."""
    a, b = scene_grid(dl, ctx, 0), scene_grid(dl, ctx, 1)
    index = dl.FeatureIndex(ctx, 64)
    options = dl.surf_options()
    na, oxa, oya, res = index.add_from_grid(0, a, IDENTITY, options)
    nb, oxb, oyb, _ = index.add_from_grid(1, b, IDENTITY, options)
    match = fm.Options(ratio=0.5, minimum_good=5, threshold=3.0, tolerance=0.1, seed=7)
    r = index.match(0, [1], match.device(dl))[0][0]
    print("key points %d / %d, status %d, good %d, inliers %d, theta %.3f deg" % (na, nb, r["status"], r["good_matches"],
                                                                                 r["inliers"], np.degrees(r["theta"])))
    assert r["status"] == fm.MATCHED and r["inliers"] >= 2 * match.minimum_good
    assert abs(abs(np.degrees(r["theta"])) - 90.0) <= 5.0
    image = dl.grid_project_to_image(a, IDENTITY)[0]
    centre = np.array([oxa + 0.5 * image.shape[1] * res, oya + 0.5 * image.shape[0] * res])
    got = np.array([r["a"] * centre[0] - r["b"] * centre[1] + r["tx"], r["b"] * centre[0] + r["a"] * centre[1] + r["ty"]])
    want = np.array([-centre[1], centre[0]])
    assert np.linalg.norm(got - want) <= match.threshold, (got, want)
    index.close()
    a.close()
    b.close()


def test_adapter_equals_binding(dl, ctx, tmp_path):
    """tests/cpp/surf_adapter.cc builds the scene's grid from a file of points, adds it twice (once turned) through
    SubmapFeatureMatcher::AddSubmap(id, grid, pose, options) and prints the second call's matched_submaps; the binding on
    the same grids gives the same numbers."""
    from dliom import synth
    libdir = os.path.join(sc.ROOT, "d-liom_amd")
    exe = str(tmp_path / "surf_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(sc.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(sc.ROOT, "tests", "cpp", "surf_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    scans = []
    for s in range(6):
        pose = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(pose, 16, 256)
        scans.append((pose[:3].astype(np.float32), np.ascontiguousarray(synth.transform_points(pose, pts), np.float32)))
    path = tmp_path / "scans.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(scans)).tobytes())
        for origin, world in scans:
            f.write(np.int32(len(world)).tobytes() + origin.tobytes() + world.tobytes())
    out = subprocess.check_output([exe, str(path)]).decode().split()
    a, b = scene_grid(dl, ctx, 0), scene_grid(dl, ctx, 1)
    index = dl.FeatureIndex(ctx, 64)
    index.add_from_grid(0, a, IDENTITY, dl.surf_options())
    index.add_from_grid(1, b, IDENTITY, dl.surf_options())
    r = index.match(1, [0], dl.feature_match_options(0.5, 5, 3.0, 0.1, 7))[0][0]
    assert r["status"] == fm.MATCHED
    assert out[0] == "1" and int(out[1]) == 0
    assert [float(v).hex() for v in out[2:5]] == [float(v).hex() for v in (r["theta"], r["tx"], r["ty"])]
    index.close()
    a.close()
    b.close()
