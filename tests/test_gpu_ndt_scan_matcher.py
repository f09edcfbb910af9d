"""dliom_ndt_scan_matcher (MatchByNDT over a stream of scans, the previous scan's cells kept on the device) against the
composition that is already pinned -- the model's filter of both scans, NdtTarget, dliom_ndt_align -- and against the
adapter's registration::MatchByNDT: bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_voxel_common as av  # noqa: E402
import ndt_common as nd  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = ("converged", "reason", "iterations", "evaluations_with_hessian", "evaluations_without_hessian", "pairs", "score",
            "transformation_probability", "fitness_count")


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


@pytest.fixture(scope="module")
def stream():
    """Four scans of the room, 16 x 128 (2048 points each), 10 ms of the corkscrew apart, and the three guesses: the
    identity, and two small rigid motions whose entries are floats, as the adapter's Matrix4f holds them.  The room is
    scaled to a quarter (8.6 m across, the motion 1 cm and 0.2 degrees a scan): at its own size 2048 points leave two 1 m
    cells with the six points NDT asks for; scaled, the filter merges 2048 points into about 1540 and the model counts 75
    valid cells and 4000 (point, cell) pairs a scan"""
    from dliom import synth
    scans = [(np.float32(0.25) * synth.scan(synth.trajectory_pose(0.30 + 0.01 * k), 16, 128)[0]).astype(np.float32) for k in range(4)]
    guesses = [np.eye(4), nd.transform_of([0.03, -0.02, 0.01, 0.002, -0.003, 0.004]),
               nd.transform_of([-0.02, 0.04, 0.0, -0.004, 0.001, 0.002])]
    guesses = [g.astype(np.float32).astype(np.float64) for g in guesses]
    for s in scans:
        s.setflags(write=False)
    return scans, guesses


@pytest.fixture(scope="module")
def composed(dl, ctx, stream):
    """Every pair by the pinned composition, computed once"""
    scans, guesses = stream
    filtered = [av.sequential(s, 0.2) for s in scans]
    out = []
    for k in range(1, len(scans)):
        target = dl.NdtTarget(ctx, filtered[k - 1])
        try:
            out.append(dl.Ndt(target).align(filtered[k], guess=guesses[k - 1]))
        finally:
            target.close()
    return out


def test_every_pair_equals_the_composition(dl, ctx, stream, composed):
    scans, guesses = stream
    matcher = dl.NdtScanMatcher(ctx)
    try:
        assert matcher.num_scans == 0 and not matcher.has_target
        assert matcher.match(scans[0]) is None  # the first scan: no result
        assert matcher.num_scans == 1 and matcher.has_target
        for k in range(1, len(scans)):
            got, want = matcher.match(scans[k], guesses[k - 1]), composed[k - 1]
            for key in COMPARED:
                assert got[key] == want[key], (k, key, got[key], want[key])
            assert got["p"].tobytes() == want["p"].tobytes() and got["transform"].tobytes() == want["transform"].tobytes(), k
            assert np.isnan(got["fitness_score"]) and got["pairs"] > 0 and got["iterations"] >= 1
        assert matcher.num_scans == len(scans)
    finally:
        matcher.close()


def test_every_pair_equals_the_adapters_match_by_ndt(dl, stream, composed, tmp_path):
    """registration::MatchByNDT (host filter, upload, a target a pair) and registration::NdtScanMatcher in a C++ program"""
    scans, guesses = stream
    libdir = os.path.join(ROOT, "d-liom_amd")
    exe = str(tmp_path / "approx_voxel_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "approx_voxel_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    paths = []
    for k, s in enumerate(scans):
        paths.append(str(tmp_path / ("scan%d.bin" % k)))
        open(paths[-1], "wb").write(s.tobytes())
    (tmp_path / "guesses.bin").write_bytes(np.concatenate([g.reshape(16) for g in guesses]).astype(np.float32).tobytes())
    subprocess.check_call([exe, "match", str(tmp_path / "guesses.bin"), str(tmp_path / "out.bin")] + paths)
    out = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(len(scans) - 1, 2, 12)
    for k, want in enumerate(composed):
        t = want["transform"].astype(np.float32)
        expected = np.concatenate([t[:3, :3].reshape(9), t[:3, 3]])
        assert out[k, 0].tobytes() == expected.tobytes(), ("MatchByNDT", k)
        assert out[k, 1].tobytes() == expected.tobytes(), ("NdtScanMatcher", k)


def test_a_failed_match_leaves_the_matcher_as_it_was(dl, ctx, stream, composed):
    scans, guesses = stream
    matcher = dl.NdtScanMatcher(ctx)
    try:
        matcher.match(scans[0])
        bad = scans[1].copy()
        bad[5, 1] = np.nan
        with pytest.raises(Exception):
            matcher.match(bad, guesses[0])
        with pytest.raises(Exception):
            matcher.match(scans[1], 2.0 * np.eye(4))  # not a rigid guess
        assert matcher.num_scans == 1 and matcher.has_target
        got = matcher.match(scans[1], guesses[0])
        assert got["transform"].tobytes() == composed[0]["transform"].tobytes()
    finally:
        matcher.close()


def test_a_matcher_destroyed_after_one_scan_leaks_nothing(dl, ctx, stream):
    scans, _ = stream
    warm = dl.NdtScanMatcher(ctx)  # the context's scratch grows on first use and stays
    warm.match(scans[0])
    warm.close()
    before = ctx.memory_stats()
    for _ in range(3):
        matcher = dl.NdtScanMatcher(ctx)
        assert matcher.match(scans[0]) is None
        matcher.close()
    assert ctx.memory_stats() == before


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_a_decoded_message_reaches_the_matcher_without_a_download(dl, ctx, n):
    """dliom_timed_cloud_points (cvtPointCloud): the xyz of a decoded message as a cloud, copied on the device, with the
    cloud's bound; another context's object is refused"""
    import ctypes as C
    import point_cloud2_common as pc
    message = pc.make_message(7 + n, pc.MODES[0], 1, n)
    timed, _, _ = message.to_library(dl).decode(ctx, pc.MODES[0], None)
    try:
        xyzt, _ = timed.download()
        cloud = dl.timed_cloud_points(ctx, timed)
        try:
            got, max_norm = cloud.download(), cloud.bounds()[0]
            xyz = np.ascontiguousarray(xyzt[:, :3], np.float32)
            assert len(xyzt) > 0 and got.tobytes() == xyz.tobytes()
            assert max_norm == np.sqrt((xyz[:, 0] * xyz[:, 0] + (xyz[:, 1] * xyz[:, 1] + xyz[:, 2] * xyz[:, 2])).max())
            if n == 4099:  # the same points, uploaded or taken from the decoded message: the same filtered cloud
                a, b = dl.approximate_voxel_filter(ctx, cloud, 0.2), dl.approximate_voxel_filter(ctx, xyz, 0.2)
                assert a.download().tobytes() == b.download().tobytes() == av.sequential(xyz, 0.2).tobytes()
                a.close()
                b.close()
        finally:
            cloud.close()
        other = dl.Context(0)
        try:
            h = C.c_void_p()
            assert dl.load_library().dliom_timed_cloud_points(other.h, timed.h, C.byref(h)) == dl.ERR_INVALID_ARGUMENT and not h.value
        finally:
            other.close()
    finally:
        timed.close()
