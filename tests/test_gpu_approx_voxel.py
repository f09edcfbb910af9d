"""dliom_cloud_approximate_voxel_filter on the device against the sequential loop of its definition
(tests/approx_voxel_common.py): bits and order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_voxel_common as av  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


def device(dl, ctx, cloud, leaf):
    out = dl.approximate_voxel_filter(ctx, cloud, leaf)
    try:
        return out.download(), out.bounds()[0]
    finally:
        out.close()


def check(dl, ctx, cloud, leaf=0.2):
    """-> the model's output; the device's equals it, and the cloud's bound is the largest norm of the centroids"""
    want = av.sequential(cloud, leaf)
    got, max_norm = device(dl, ctx, cloud, leaf)
    assert got.shape == want.shape, (got.shape, want.shape)
    differs = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert differs.size == 0, (differs[:8], got[differs[:3]], want[differs[:3]])
    if len(want):
        sq = want[:, 0] * want[:, 0] + (want[:, 1] * want[:, 1] + want[:, 2] * want[:, 2])
        assert max_norm == np.sqrt(sq.max())
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 65537])
def test_sizes_at_chunk_and_grid_boundaries(dl, ctx, n):
    """A workgroup is 256 lanes; 65 537 points are 257 of them.  The cloud churns: 3 m a side at 0.2 m, 3375 voxels"""
    want = check(dl, ctx, av.random_cloud(n, seed=n, scale=1.5))
    assert len(want) == n if n <= 2 else 0 < len(want) <= n


@pytest.mark.parametrize("leaf", [0.2, 0.3])
def test_random_and_clustered_clouds(dl, ctx, leaf):
    for seed, scale, clustered in ((1, 0.3, False), (2, 3.0, False), (3, 30.0, False), (4, 3.0, True), (5, 30.0, True)):
        check(dl, ctx, av.random_cloud(3001, seed, scale, clustered), leaf)


def test_one_voxel_is_one_long_sequential_sum(dl, ctx):
    assert len(check(dl, ctx, av.one_voxel(4097))) == 1


def test_alternating_collision_every_point_evicts(dl, ctx):
    assert len(check(dl, ctx, av.alternating(100))) == 100


def test_a_b_a_emits_a_twice(dl, ctx):
    assert len(check(dl, ctx, av.a_b_a())) == 3


def test_final_flush_order(dl, ctx):
    """All 512 slots occupied at the end, in stream order shuffled; against a single slot occupied at the end"""
    assert len(check(dl, ctx, av.every_slot())) == av.SLOTS
    assert len(check(dl, ctx, av.every_slot(shuffled=False))) == av.SLOTS
    assert len(check(dl, ctx, av.alternating(7))) == 7  # six evictions, then the one occupied slot


@pytest.mark.parametrize("leaf", [0.2, 0.3])
def test_faces_negative_coordinates_and_an_ulp_either_side(dl, ctx, leaf):
    check(dl, ctx, av.faces(leaf), leaf)


def test_indices_where_the_hash_wraps(dl, ctx):
    check(dl, ctx, av.wrapping())
    edge = np.float32(2147483520.0)  # the largest float below 2^31: leaf 1 makes it the index
    check(dl, ctx, np.array([[edge, -2147483648.0, 0.5], [0.5, 0.5, edge], [edge, -2147483648.0, 0.25]], np.float32), 1.0)


def test_a_scan_in_ring_order(dl, ctx):
    """20 480 points of the room, azimuth-major as a driver delivers them: neighbours share voxels, runs are long near
    the sensor and short far from it"""
    from dliom import synth
    cloud = synth.scan(synth.trajectory_pose(0.3), 32, 640)[0]
    want = check(dl, ctx, cloud)
    assert len(cloud) == 20480 and 2000 < len(want) < len(cloud)


def test_refusals(dl, ctx):
    L = dl.load_library()
    good = av.random_cloud(300, 9)
    h = C.c_void_p()

    def status(points, leaf, context=None):
        cloud = dl.PointCloud(ctx, points)
        try:
            st = L.dliom_cloud_approximate_voxel_filter((context or ctx).h, cloud.h, C.c_float(leaf), C.byref(h))
            assert st != dl.OK and not h.value
            return st
        finally:
            cloud.close()

    for k, bad in enumerate(([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [5e8, 0, 0], [0, -5e8, 0])):
        cloud = good.copy()
        cloud[17 * k + 3] = bad
        assert status(cloud, 0.2) == dl.ERR_INVALID_ARGUMENT, bad
    for leaf in (0.0, -0.2, float("nan")):
        assert status(good, leaf) == dl.ERR_INVALID_ARGUMENT, leaf
    other = dl.Context(0)
    try:
        assert status(good, 0.2, other) == dl.ERR_INVALID_ARGUMENT  # another context's cloud
    finally:
        other.close()
    check(dl, ctx, good)  # the context is usable afterwards


def test_the_adapters_host_class_equals_the_device(dl, tmp_path):
    """registration::ApproximateVoxelGrid and the device call on one cloud, in a C++ program"""
    libdir = os.path.join(ROOT, "d-liom_amd")
    exe = str(tmp_path / "approx_voxel_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "approx_voxel_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    cloud = av.random_cloud(5000, 21, 3.0, clustered=True)
    (tmp_path / "in.bin").write_bytes(cloud.tobytes())
    subprocess.check_call([exe, "filter", "0.2", str(tmp_path / "in.bin"), str(tmp_path / "host.bin"), str(tmp_path / "device.bin")])
    host, dev = (tmp_path / "host.bin").read_bytes(), (tmp_path / "device.bin").read_bytes()
    assert host == dev and host == av.sequential(cloud, 0.2).tobytes() and len(host) > 0
