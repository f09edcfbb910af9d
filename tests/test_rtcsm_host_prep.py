"""The host prep of an RTCSM3D match (d-liom_amd/csrc/rtcsm_candidates.h): the candidate tables built in place, the
rotations in one vectorised loop.

Without a GPU: tests/cpp/rtcsm_candidates_check.cc holds rot[i], trans[j], t_norm and r_angle of the new path against the
scalar functions of host_math.h bit for bit, on 1 000 random initial poses and windows with A = 1, 5 and 9; built with the
library's host flags and once more, stand-alone, with -fsanitize=address,undefined.

With one (-m gpu): Match -> Ceres -> insert (hi + lo) over 12 scans of 16 x 64 returns on a 10 cm grid against the CPU
oracle after every scan, once with bench.py's search (the LDS-box kernel, whose pre-pass carries the tables) and once
with a search the box kernel refuses as small (the dense kernel behind rtcsm_prep_kernel)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import (DEFAULT_CSM, DEFAULT_RTCSM, FREE, build_device_scene, device_cells_sorted, device_grid_to_oracle,
                     oracle_cells_sorted, pose_distance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "rtcsm_candidates_check.cc")
THREADS = min(8, os.cpu_count() or 1)
SMALL_RTCSM = dict(DEFAULT_RTCSM, angular_search_window=float(np.deg2rad(0.3)))


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-o", exe, CHECK])
    out = subprocess.check_output([exe]).decode().split()
    print(" ".join(out))
    return out


def test_host_prep_equals_the_scalar_functions(tmp_path):
    out = _build_and_run(tmp_path, "rtcsm_candidates_check", ["-O3"])  # the library's host flags: the loop is vectorised
    assert out[:3] == ["ok", "cases", "1000"]
    # A = 1, 5, 9 in turn: 334 windows of 27 rotations, 333 of 1 331 and 333 of 6 859
    assert int(out[4]) == 334 * 27 + 333 * 1331 + 333 * 6859


def test_host_prep_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "rtcsm_candidates_check_san",
                         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out[:3] == ["ok", "cases", "1000"]


def test_the_searches_of_the_gpu_tests(orc):
    """The sequences below need >= 2^24 candidate-point pairs and >= 8 translations for the box kernel, and fewer pairs
    for its refusal: checked on the CPU for the twelve clouds (the window depends on the scan's range alone)."""
    from dliom import synth
    for k in range(12):
        pts, _ = synth.scan(synth.trajectory_pose(0.1 * (6 + k)), 16, 64, centers=synth.bubbles())
        assert len(pts) == 1024
        for opts, box in ((DEFAULT_RTCSM, True), (SMALL_RTCSM, False)):
            w = orc.rtcsm3d_window(opts, 0.1, pts)
            T, R = (2 * w["linear_window"] + 1) ** 3, (2 * w["angular_window"] + 1) ** 3
            print(k, w, T, R, T * R * len(pts))
            assert T >= 8
            assert (T * R * len(pts) >= 2 ** 24) == box


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    assert dliom.device_count() > 0, "no HIP device: the GPU tests must not pass on a fallback"
    return dliom


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["box", "small"])
def test_twelve_scans_against_the_oracle(dl, orc, search):
    """After every scan: RTCSM3D's pose and score equal the oracle's bit for bit, Ceres' pose lies within the 1e-6 m / rad
    of tests/test_gpu_full_size.py (Cholesky against the oracle's QR), and both grids, inserted into at the device's pose
    on either side, are bit-equal.  Every match after the first finds its rotation table and its staging in place."""
    opts = DEFAULT_RTCSM if search == "box" else SMALL_RTCSM
    ctx = dl.Context(0)
    ins, g_hi, g_lo, scans = build_device_scene(dl, ctx, 16, 64, 0.10, 0.45, map_scans=6, num_scans=12)
    og_hi, og_lo = device_grid_to_oracle(orc, g_hi), device_grid_to_oracle(orc, g_lo)
    rt = dl.RealTimeCorrelativeScanMatcher3D(ctx, opts)
    cs = dl.CeresScanMatcher3D(ctx, DEFAULT_CSM)
    for k, sc in enumerate(scans):
        score, p1 = rt.Match(sc["init"], sc["cloud"], g_hi)
        st = rt.last_stats()
        if search == "box":
            assert st.score_kernel == 3 and st.box_kernel_status == dl.BOX_RAN, (k, st.score_kernel, st.box_kernel_status)
            assert st.window.num_translations >= 8 and st.window.num_candidates * st.num_points >= 2 ** 24
        else:
            assert st.score_kernel == 2 and st.box_kernel_status == dl.BOX_REFUSED_SMALL, (k, st.score_kernel, st.box_kernel_status)
        ref = orc.rtcsm3d_match_parallel(opts, sc["init"], sc["pts"], og_hi, threads=THREADS)
        assert st.best_index == ref["best_index"], (k, st.best_index, ref["best_index"])
        assert np.float32(score).tobytes() == np.float32(ref["score"]).tobytes(), k
        assert np.array_equal(p1, ref["pose"]), k
        p2, summ = cs.Match(sc["init"][:3], p1, [(sc["cloud"], g_hi), (sc["cloud"], g_lo)])
        r2 = orc.csm3d_match(DEFAULT_CSM, sc["init"][:3], ref["pose"], [(sc["pts"], og_hi), (sc["pts"], og_lo)])
        dt, dr = pose_distance(p2, r2["pose"])
        assert dt <= 1e-6 and dr <= 1e-6, (k, dt, dr)
        pf = np.asarray(p2, dtype=np.float32)
        dl.insert_cloud_multi(ins, sc["cloud"], [(g_hi, [pf], 20.0), (g_lo, [pf], 0.0)])
        world = orc.transform_points(pf, sc["pts"])
        origin = orc.transform_points(pf, np.zeros((1, 3), np.float32))[0]
        d = (world - origin).astype(np.float32)  # FilterRangeDataByMaxRange: float norm, Eigen's reduction order
        nrm = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), dtype=np.float32)
        og_hi.insert_tables(origin, world[nrm <= np.float32(20.0)], ins.hit_table, ins.miss_table, FREE)
        og_lo.insert_tables(origin, world, ins.hit_table, ins.miss_table, FREE)
        for dg, og in ((g_hi, og_hi), (g_lo, og_lo)):
            dk, dv = device_cells_sorted(dg)
            ok, ov = oracle_cells_sorted(og)
            assert np.array_equal(dk, ok) and np.array_equal(dv, ov), k
    assert rt.box_error() == 0
    for sc in scans:
        sc["cloud"].close()
    g_hi.close()
    g_lo.close()
    ctx.close()
