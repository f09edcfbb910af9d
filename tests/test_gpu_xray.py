"""X-ray projections on the device (dliom_grid_xray_texture, dliom_grid_project_to_image) against the CPU model of
the reference's arithmetic (tests/cpp/xray_model.cc), byte for byte: sizes, resolution, slice pose / ox, oy and every
pixel, on oracle-built and front-end submaps, grown grids, tall columns, empty projections and several poses."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import build_oracle_submap, to_device_grid
from test_xray_host import IDENTITY, MODEL_SRC, ROOT, run_model

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
    exe = str(tmp_path_factory.mktemp("xray_model") / "xray_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def yaw_pose(t, yaw):
    return [t[0], t[1], t[2], np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]


def random_pose(seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return list(rng.uniform(-30, 30, size=3)) + list(q)


POSES = [IDENTITY, yaw_pose((1.25, -3.5, 0.4), 0.7), random_pose(11), random_pose(12)]


def same_texture(a, b):
    return a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes() and a[4].shape == b[4].shape and np.array_equal(a[4], b[4])


def same_image(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and (a[1], a[2], a[3]) == (b[1], b[2], b[3])


def check(dl, model, grid, pose, tmp_path):
    proto = grid.to_proto()
    dev_t = dl.grid_xray_texture(grid, pose)
    ref_t = run_model(model, "texture", proto, pose, tmp_path)
    assert same_texture(dev_t, ref_t), (dev_t[:4], ref_t[:4])
    dev_i = dl.grid_project_to_image(grid, pose)
    ref_i = run_model(model, "image", proto, pose, tmp_path)
    assert same_image(dev_i, ref_i), (dev_i[0].shape, dev_i[1:], ref_i[0].shape, ref_i[1:])
    return dev_t, dev_i


@pytest.mark.parametrize("resolution", [0.10, 0.45])
def test_oracle_submaps_equal_model(dl, ctx, orc, model, tmp_path, resolution):
    og = build_oracle_submap(orc, resolution, num_scans=6, beams=16, azimuths=256)
    g = to_device_grid(dl, ctx, og)
    for pose in POSES:
        tex, img = check(dl, model, g, pose, tmp_path)
        assert tex[0] > 10 and tex[1] > 10 and (tex[4][..., 1] > 0).any()  # a real picture, not an empty one
        assert (img[0] != 224).any()
    g.close()


def test_front_end_submaps_equal_model(dl, ctx, model, tmp_path):
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    fe = dl.LocalTrajectoryBuilder3D(ctx, FRONT_END_OPTS)
    gravity = np.array([1.0, 0, 0, 0])
    finished = None
    for s in range(14):
        truth = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(truth, 16, 256)
        r = fe.match(synth.perturb_pose(truth, 0.03, 0.2, seed=200 + s), np.zeros(3, np.float32), pts)
        fe.insert(int(s * 1e6), r["pose_estimate"], gravity)
        if fe.num_finished_submaps() > 0:
            finished = fe.take_finished_submap()
            break
    assert finished is not None
    active = fe.active_submap(0)
    for sub in (finished, active):
        for grid in (sub["hi"], sub["lo"]):
            check(dl, model, grid, list(sub["local_pose"]), tmp_path)
        check(dl, model, sub["hi"], POSES[2], tmp_path)
    finished["hi"].close()
    finished["lo"].close()
    fe.close()


def wall_grid(dl, ctx, resolution):
    """A wall at negative x far enough out to grow the grid to bits >= 4, columns of 60 cells with varied values, and
    a few scattered cells: the per-pixel float sums run over dozens of terms in iterator order."""
    L = dl.load_library()
    rng = np.random.default_rng(5)
    xs, ys, zs = np.meshgrid(np.arange(-420, -400), np.arange(-30, 10), np.arange(-30, 30), indexing="ij")
    cells = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], axis=1)
    cells = np.concatenate([cells, rng.integers(-300, 300, size=(2000, 3))])
    probs = rng.uniform(0.3, 0.9, size=len(cells)).astype(np.float32)
    values = np.array([L.dliom_probability_to_value(C.c_float(p)) for p in probs], dtype=np.uint16)
    g = dl.HybridGrid(ctx, resolution)
    g.set_values(cells, values)
    return g


def test_grown_grid_with_tall_columns_equals_model(dl, ctx, model, tmp_path):
    g = wall_grid(dl, ctx, 0.05)
    assert g.bits >= 4
    for pose in (IDENTITY, yaw_pose((0.0, 0.0, 0.0), np.pi / 2), POSES[3]):
        tex, img = check(dl, model, g, pose, tmp_path)
    assert (img[0] > 0).any()
    g.close()


def test_empty_projections(dl, ctx, model, tmp_path):
    L = dl.load_library()
    empty = dl.HybridGrid(ctx, 0.1)
    low = dl.HybridGrid(ctx, 0.1)
    low.set_values([(0, 0, 0), (5, -3, 2)], [L.dliom_probability_to_value(C.c_float(0.5))] * 2)
    for g in (empty, low):
        for pose in (IDENTITY, POSES[2]):
            tex, img = check(dl, model, g, pose, tmp_path)
            assert tex[:2] == (0, 0) and img[0].shape == (0, 0)
        g.close()


def test_size_query_and_small_buffer(dl, ctx, orc, tmp_path):
    L = dl.load_library()
    og = build_oracle_submap(orc, 0.45, num_scans=2, beams=8, azimuths=64)
    g = to_device_grid(dl, ctx, og)
    pose = (C.c_double * 7)(*POSES[1])
    full_t = dl.grid_xray_texture(g, POSES[1])
    full_i = dl.grid_project_to_image(g, POSES[1])
    w, h, res, ox, oy = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_double()
    sl = (C.c_double * 7)()
    u8 = C.POINTER(C.c_uint8)
    assert L.dliom_grid_xray_texture(g.h, pose, None, 0, C.byref(w), C.byref(h), C.byref(res), sl) == dl.OK
    assert (w.value, h.value, res.value) == full_t[:3] and np.array(sl[:]).tobytes() == full_t[3].tobytes()
    need = 2 * w.value * h.value
    small = (C.c_uint8 * need)()
    w.value = h.value = -1
    assert L.dliom_grid_xray_texture(g.h, pose, C.cast(small, u8), need - 1, C.byref(w), C.byref(h), C.byref(res),
                                     sl) == dl.ERR_CAPACITY
    assert (w.value, h.value) == full_t[:2]
    assert not any(small)  # nothing written
    assert L.dliom_grid_project_to_image(g.h, pose, None, 0, C.byref(w), C.byref(h), C.byref(ox), C.byref(oy),
                                         C.byref(res)) == dl.OK
    assert (h.value, w.value) == full_i[0].shape and (ox.value, oy.value, res.value) == full_i[1:]
    need = w.value * h.value
    w.value = h.value = -1
    assert L.dliom_grid_project_to_image(g.h, pose, C.cast(small, u8), need - 1, C.byref(w), C.byref(h), C.byref(ox),
                                         C.byref(oy), C.byref(res)) == dl.ERR_CAPACITY
    assert (h.value, w.value) == full_i[0].shape
    assert L.dliom_grid_xray_texture(g.h, None, None, 0, C.byref(w), C.byref(h), C.byref(res), sl) == dl.ERR_INVALID_ARGUMENT
    g.close()


def test_cpp_adapter_equals_python(dl, ctx, orc, tmp_path):
    """Submap3D::ToResponseProto (version, high then low texture) and ProjectToCvMat of the C++ adapter, run in a process
    of its own on grids read from the same protos."""
    exe = str(tmp_path / "xray_adapter")
    libdir = os.path.join(ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "xray_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
    grids = [to_device_grid(dl, ctx, build_oracle_submap(orc, r, num_scans=3)) for r in (0.10, 0.45)]
    protos = [g.to_proto() for g in grids]
    for k, p in enumerate(protos):
        (tmp_path / ("g%d.pb" % k)).write_bytes(p)
    pose = POSES[2]
    out = tmp_path / "adapter.bin"
    r = subprocess.run([exe, str(tmp_path / "g0.pb"), str(tmp_path / "g1.pb"), "7"] + [repr(float(v)) for v in pose] +
                       [str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = out.read_bytes()
    assert struct.unpack_from("<i", data)[0] == 7
    at = 4
    same = [dl.HybridGrid.from_proto(ctx, p) for p in protos]
    for g in same:
        want = dl.grid_xray_texture(g, pose)
        w, h, res = struct.unpack_from("<iid", data, at)
        slice_pose = np.array(struct.unpack_from("<7d", data, at + 16))
        cells = np.frombuffer(data, dtype=np.uint8, count=2 * w * h, offset=at + 72).reshape(h, w, 2)
        assert same_texture((w, h, res, slice_pose, cells), want)
        at += 72 + 2 * w * h
    rows, cols = struct.unpack_from("<ii", data, at)
    ox, oy, res = struct.unpack_from("<3d", data, at + 8)
    img = np.frombuffer(data, dtype=np.uint8, count=rows * cols, offset=at + 32).reshape(rows, cols)
    assert same_image((img, ox, oy, res), dl.grid_project_to_image(same[0], pose))
    assert at + 32 + rows * cols == len(data)
    for g in grids + same:
        g.close()
