"""Submap feature matching without a GPU: the CPU model (tests/cpp/feature_match_model.cc) alone -- against a planted
similarity, against an independent least-squares fit, on its hypothesis counts and on the honesty of the parity cases --
and the new names, struct layouts and adapter."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import least_squares

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_match_common as fc  # noqa: E402


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("feature_match_model")
    return fc.build_model(d), d


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_recovers_planted_similarity(model):
    """theta = 0.7, t = (12, -7), 40 % outliers, noise-free inliers: the refit is the planted transform to 1e-9.  Float
    points are free of noise only where the `to` points are exact floats: fc.ransac_points(exact=True) puts `from` on a
    1/16 m lattice and rounds cos / sin of 0.7 to 12 fractional bits (theta is then 0.7 to 2e-5, the scale 1 to 1e-4)."""
    exe, d = model
    p, P, outlier, planted = fc.ransac_points(200, 31, exact=True)
    assert outlier.sum() == 80
    r, mask, _ = fc.model_ransac(exe, d, p, P, fc.THRESHOLD, 3)
    got = np.array([r["a"], r["b"], r["tx"], r["ty"]])
    print("planted", planted, "got", got, "inliers", r["inliers"])
    assert r["status"] == fc.MATCHED and r["inliers"] == 120 and np.array_equal(mask == 1, ~outlier)
    assert np.abs(got - np.array(planted)).max() <= 1e-9
    assert abs(r["theta"] - fc.THETA) <= 1e-4 and abs(r["scale"] - 1.0) <= 1e-3
    assert r["scale"] == np.sqrt(r["a"] ** 2 + r["b"] ** 2) and abs(r["theta"] - np.arctan2(r["b"], r["a"])) <= 1e-15


def test_refit_is_the_least_squares_fit(model):
    """The refit against scipy.optimize.least_squares on the inliers' reprojection residuals, to 1e-9."""
    exe, d = model
    p, P, _, _ = fc.ransac_points(200, 71)
    r, mask, _ = fc.model_ransac(exe, d, p, P, fc.THRESHOLD, 1)
    assert r["status"] == fc.MATCHED and 100 < r["inliers"] == mask.sum() < 200
    pi, Pi = p[mask == 1].astype(np.float64), P[mask == 1].astype(np.float64)

    def residuals(x):
        return (fc.apply(x[0], x[1], x[2:], pi) - Pi).ravel()
    sol = least_squares(residuals, np.array([1.0, 0.0, 0.0, 0.0]), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    got = np.array([r["a"], r["b"], r["tx"], r["ty"]])
    print("model", got, "scipy", sol.x, "difference", np.abs(got - sol.x).max())
    assert np.abs(got - sol.x).max() <= 1e-9


def test_hypothesis_counts(model):
    """M = 63 enumerates all 1 953 pairs, M = 64 samples 2 000; below, all pairs."""
    exe, d = model
    for M, want in ((2, 1), (5, 10), (63, 1953), (64, 2000), (200, 2000)):
        p, P, threshold, seed = fc.RANSAC_CASES["m%d_seed1" % M]
        r, _, _ = fc.model_ransac(exe, d, p, P, threshold, seed)
        assert r["num_hypotheses"] == want and 0 <= r["hypothesis"] < want
    # enumeration is lexicographic and ties go to the lowest h: three exact matches in front of two outliers that agree
    # with nothing win as (0, 1), h = 0; behind them, as (2, 3), h = 4 + 3
    p = np.array([[0, 0], [10, 0], [0, 10], [50, 7], [20, 20]], np.float32)
    P = np.array([[1, 1], [11, 1], [1, 11], [9, -50], [70, 70]], np.float32)
    r, mask, _ = fc.model_ransac(exe, d, p, P, 0.5, 0)
    assert r["hypothesis"] == 0 and list(mask) == [1, 1, 1, 0, 0]
    order = [3, 4, 0, 1, 2]
    r, mask, _ = fc.model_ransac(exe, d, p[order], P[order], 0.5, 0)
    assert r["hypothesis"] == 7 and list(mask) == [0, 0, 1, 1, 1]
    assert np.abs(np.array([r["a"], r["b"], r["tx"], r["ty"]]) - [1.0, 0.0, 1.0, 1.0]).max() <= 1e-12


def test_two_seeds_two_answers(model):
    exe, d = model
    a = fc.model_ransac(exe, d, *fc.RANSAC_CASES["m200_other_seed_a"])[0]
    b = fc.model_ransac(exe, d, *fc.RANSAC_CASES["m200_other_seed_b"])[0]
    assert a["status"] == b["status"] == fc.MATCHED and a["hypothesis"] != b["hypothesis"]


def test_scale_and_no_model_cases(model):
    exe, d = model
    near = fc.model_ransac(exe, d, *fc.RANSAC_CASES["m200_scale_1.05"])[0]
    far = fc.model_ransac(exe, d, *fc.RANSAC_CASES["m200_scale_1.2"])[0]
    assert abs(near["scale"] - 1.05) < 0.01 and abs(near["scale"] - 1) <= fc.SCALE_TOLERANCE < abs(far["scale"] - 1)
    assert abs(far["scale"] - 1.2) < 0.01
    none = fc.model_ransac(exe, d, *fc.RANSAC_CASES["m64_same_from"])
    assert none[0]["status"] == fc.NO_MODEL and none[0]["hypothesis"] == -1 and not none[1].any()


@pytest.mark.parametrize("name", list(fc.RANSAC_CASES))
def test_ransac_cases_are_honest(model, name):
    """No evaluated (hypothesis, match) of a parity case lies within 1e-9 (relative) of the inlier threshold."""
    exe, d = model
    r, _, margin = fc.model_ransac(exe, d, *fc.RANSAC_CASES[name])
    print(name, "threshold_margin", margin, "status", r["status"], "inliers", r["inliers"])
    assert margin > 1e-9


@pytest.mark.parametrize("name", list(fc.MATCH_CASES))
def test_match_cases_are_honest(model, name):
    """No ratio test and no inlier test of a parity case is decided within 1e-9 (relative) of its bound; and the cases
    hold the statuses they are there for."""
    exe, d = model
    sets, query, train, options = fc.MATCH_CASES[name]
    results, ratio_margin, threshold_margin, _ = fc.model_match(exe, d, sets, query, train, options)
    print(name, "ratio_margin", ratio_margin, "threshold_margin", threshold_margin, list(results["status"]), list(results["good_matches"]))
    assert ratio_margin > 1e-9 and threshold_margin > 1e-9
    if name == "scene":
        assert list(results["status"]) == [fc.TOO_FEW_KEYPOINTS, fc.TOO_FEW_KEYPOINTS, fc.TOO_FEW_GOOD_MATCHES, fc.MATCHED, fc.MATCHED,
                                           fc.SCALE_REJECTED, fc.TOO_FEW_GOOD_MATCHES]
        assert results["good_matches"][3] > 63 > results["good_matches"][4] >= options.minimum_good
        assert abs(results["theta"][3] - fc.THETA) < 0.01 and abs(results["tx"][3] - 12) < 0.3 and abs(results["ty"][3] + 7) < 0.3
        assert abs(results["scale"][4] - 1.05) < 0.01 and abs(results["scale"][5] - 1.2) < 0.01
    if name == "same_keypoints":
        assert list(results["status"]) == [fc.NO_MODEL] and results["good_matches"][0] > 63
    if name == "capacity":
        assert list(results["status"]) == [fc.ERR_CAPACITY, fc.MATCHED] and results["good_matches"][0] == fc.MAX_GOOD + 4


def test_model_knn_spot_checks(model):
    """The model's nearest neighbours against numpy on a case without ties, and its tie rule on duplicated descriptors."""
    exe, d = model
    rng = np.random.RandomState(1)
    q, t = fc.unit_descriptors(rng, 40, 64), fc.unit_descriptors(rng, 70, 64)
    j0, j1, d0, d1 = fc.model_knn(exe, d, q, t)
    dist = np.linalg.norm(q[:, None, :].astype(np.float64) - t[None, :, :], axis=2)
    order = np.argsort(dist, axis=1)
    assert np.array_equal(j0, order[:, 0]) and np.array_equal(j1, order[:, 1])
    assert np.allclose(d0, dist[np.arange(40), order[:, 0]], rtol=1e-6) and np.allclose(d1, dist[np.arange(40), order[:, 1]], rtol=1e-6)
    t2 = np.concatenate([t[5:6], t, t[5:6]])  # rows 0, 6 and 71 are one descriptor
    j0, j1, d0, d1 = fc.model_knn(exe, d, t[5:6], t2)
    assert (j0[0], j1[0], d0[0], d1[0]) == (0, 6, 0.0, 0.0)


def test_constants_and_symbols(dl):
    header = open(os.path.join(fc.ROOT, "include", "dliom.h")).read()
    for name, value in (("RANSAC_HYPOTHESES", fc.HYPOTHESES), ("MAX_GOOD", fc.MAX_GOOD), ("TRAIN_CHUNK", fc.CHUNK)):
        assert int(re.search(r"#define DLIOM_FEATURE_%s (\d+)" % name, header).group(1)) == value == getattr(dl, "FEATURE_" + name)
    names = {n for n, _, _ in dl.SYMBOLS}
    for n in ("create", "destroy", "size", "memory_stats", "add", "remove", "match", "knn"):
        assert "dliom_feature_index_" + n in names and getattr(dl.load_library(), "dliom_feature_index_" + n) is not None
    assert "dliom_feature_ransac" in names and dl.load_library().dliom_feature_ransac is not None
    assert "parity unpinned against opencv" in header.lower()


def test_argument_checks(dl):
    L = dl.load_library()
    h = C.c_void_p()
    assert L.dliom_feature_index_create(None, 64, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_index_size(None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_index_add(None, 1, None, None, 0, 0.0, 0.0, 0.1) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_index_remove(None, 1) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_index_match(None, 1, None, 0, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_index_knn(None, 1, 2, None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_feature_ransac(None, None, None, 2, 1.0, 0, None, None) == dl.ERR_INVALID_ARGUMENT


def test_struct_layouts_match_header(dl, tmp_path):
    src = tmp_path / "sizes.c"
    names = ["dliom_feature_match_options", "dliom_submap_match", "dliom_feature_match_stats", "dliom_feature_ransac_result",
             "dliom_feature_index_memory"]
    src.write_text('#include <stdio.h>\n#include "dliom.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * len(names)), ", ".join("sizeof(%s)" % n for n in names)))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fc.ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(t) for t in (dl.FeatureMatchOptions, dl.SubmapMatch, dl.FeatureMatchStats, dl.FeatureRansacResult,
                                         dl.FeatureIndexMemory)]
    assert fc.SUBMAP_MATCH.itemsize == C.sizeof(dl.SubmapMatch) and fc.RANSAC_RESULT.itemsize == C.sizeof(dl.FeatureRansacResult)
    assert len(fc.Options().pack()) == C.sizeof(dl.FeatureMatchOptions)


def test_adapter_compiles(dl, tmp_path):
    """tests/cpp/feature_match_adapter.cc (mapping::constraints::SubmapFeatureMatcher) builds with plain g++."""
    libdir = os.path.join(fc.ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(fc.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", str(tmp_path / "feature_match_adapter"),
                           os.path.join(fc.ROOT, "tests", "cpp", "feature_match_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
