"""Shared by tests/test_feature_match_host.py, tests/test_gpu_feature_match.py and tools/feature_match_bench.py: builds and
runs the CPU model (tests/cpp/feature_match_model.cc), makes the feature sets and holds the fixed case lists."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))

MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "feature_match_model.cc")
SUBMAP_MATCH = np.dtype([("key", "<i8"), ("status", "<i4"), ("good_matches", "<i4"), ("inliers", "<i4"), ("hypothesis", "<i4"),
                         ("a", "<f8"), ("b", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("scale", "<f8"), ("theta", "<f8")])
RANSAC_RESULT = np.dtype([("status", "<i4"), ("inliers", "<i4"), ("hypothesis", "<i4"), ("num_hypotheses", "<i4"), ("a", "<f8"),
                          ("b", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("scale", "<f8"), ("theta", "<f8")])
MATCHED, TOO_FEW_KEYPOINTS, TOO_FEW_GOOD_MATCHES, NO_MODEL, SCALE_REJECTED = range(5)
ERR_CAPACITY = -9
HYPOTHESES, MAX_GOOD, CHUNK = 2000, 4096, 64  # dliom.h; tests/test_feature_match_host.py checks them against the header


def build_model(directory):
    """The model, with hardware fused multiply-add where the machine has it (fmaf is correctly rounded either way; the
    library call is several times slower)."""
    exe = os.path.join(str(directory), "feature_match_model")
    fma = []
    try:
        with open("/proc/cpuinfo") as f:
            if any(line.startswith("flags") and " fma " in line + " " for line in f):
                fma = ["-mfma"]
    except OSError:
        pass
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + fma +
                          ["-I", os.path.join(ROOT, "include"), "-o", exe, MODEL_SRC])
    return exe


def _run(exe, directory, payload):
    src, dst = os.path.join(str(directory), "fm_in.bin"), os.path.join(str(directory), "fm_out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        return f.read()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def model_knn(exe, directory, query, train):
    """-> (j0, j1, d0, d1)"""
    q, t = _f32(query), _f32(train)
    nq, nt, D = len(q), len(t), q.shape[1]
    data = _run(exe, directory, struct.pack("<4i", 0, D, nq, nt) + q.tobytes() + t.tobytes())
    assert len(data) == 16 * nq
    return (np.frombuffer(data, "<i4", nq, 0), np.frombuffer(data, "<i4", nq, 4 * nq), np.frombuffer(data, "<f4", nq, 8 * nq),
            np.frombuffer(data, "<f4", nq, 12 * nq))


def model_ransac(exe, directory, from_xy, to_xy, threshold, seed):
    """-> (result: a RANSAC_RESULT record, mask (M,) uint8, threshold_margin)"""
    p, q = _f32(from_xy).reshape(-1, 2), _f32(to_xy).reshape(-1, 2)
    data = _run(exe, directory, struct.pack("<2idQ", 1, len(p), threshold, seed) + p.tobytes() + q.tobytes())
    n = RANSAC_RESULT.itemsize
    assert len(data) == n + 8 + len(p)
    return (np.frombuffer(data, RANSAC_RESULT, 1, 0)[0], np.frombuffer(data, np.uint8, len(p), n + 8).copy(),
            struct.unpack_from("<d", data, n)[0])


class FeatureSet:
    def __init__(self, descriptors, keypoints, ox, oy, resolution):
        self.descriptors, self.keypoints = _f32(descriptors), _f32(keypoints).reshape(-1, 2)
        assert len(self.descriptors) == len(self.keypoints)
        self.ox, self.oy, self.resolution = float(ox), float(oy), float(resolution)

    def __len__(self):
        return len(self.keypoints)


class Options:
    def __init__(self, ratio=0.7, minimum_good=10, threshold=3.0, tolerance=0.1, seed=7):
        self.ratio, self.minimum_good, self.threshold, self.tolerance, self.seed = ratio, minimum_good, threshold, tolerance, seed

    def pack(self):  # dliom_feature_match_options
        return struct.pack("<d2i2dQ", self.ratio, self.minimum_good, 0, self.threshold, self.tolerance, self.seed)

    def device(self, dl):
        return dl.feature_match_options(self.ratio, self.minimum_good, self.threshold, self.tolerance, self.seed)


def model_match(exe, directory, sets, query, train, options):
    """sets: a list of FeatureSet; query, train: indices into it -> (results: SUBMAP_MATCH array whose key is the index,
    ratio_margin, threshold_margin, seconds)"""
    D = sets[query].descriptors.shape[1]
    parts = [struct.pack("<5i", 2, D, len(sets), query, len(train)), options.pack(), np.asarray(train, "<i4").tobytes()]
    for s in sets:
        parts += [struct.pack("<2i3d", len(s), 0, s.ox, s.oy, s.resolution), s.descriptors.tobytes(), s.keypoints.tobytes()]
    data = _run(exe, directory, b"".join(parts))
    n = SUBMAP_MATCH.itemsize * len(train)
    assert len(data) == n + 24
    return (np.frombuffer(data, SUBMAP_MATCH, len(train), 0).copy(),) + struct.unpack_from("<3d", data, n)


# ---- data ----------------------------------------------------------------------------------------------------------------
def unit_descriptors(rng, n, D):
    d = rng.normal(size=(n, D))
    return _f32(d / np.linalg.norm(d, axis=1)[:, None])


def similarity(theta, scale=1.0):
    return scale * np.cos(theta), scale * np.sin(theta)


def apply(a, b, t, p):
    return np.stack([a * p[:, 0] - b * p[:, 1] + t[0], b * p[:, 0] + a * p[:, 1] + t[1]], axis=1)


THETA, TRANSLATION, OUTLIERS, NOISE, THRESHOLD = 0.7, (12.0, -7.0), 0.4, 0.15, 3.0


def ransac_points(M, seed, noise=NOISE, scale=1.0, outliers=OUTLIERS, exact=False):
    """M matches in a 60 m square: `to` = the planted similarity of `from` plus noise; a share of them are outliers with a
    random `to`.  exact: `from` on a 1/16 m lattice and cos / sin rounded to 12 fractional bits, so that the inliers' `to`
    points are exact floats -- the one way float points are free of noise -> (from, to, is_outlier, (a, b, tx, ty))"""
    rng = np.random.RandomState(seed)
    a, b = similarity(THETA, scale)
    p = rng.uniform(0, 60, size=(M, 2))
    if exact:
        a, b = np.round(a * 4096) / 4096, np.round(b * 4096) / 4096
        p = np.round(p * 16) / 16
        noise = 0.0
    P = apply(a, b, TRANSLATION, p) + rng.normal(0, 1, size=(M, 2)) * noise
    out = np.zeros(M, bool)
    out[rng.permutation(M)[:int(round(outliers * M))]] = True
    P[out] = rng.uniform(-40, 80, size=(int(out.sum()), 2))
    if exact:
        assert np.array_equal(_f32(P[~out]).astype(np.float64), P[~out])
    return _f32(p), _f32(P), out, (a, b, TRANSLATION[0], TRANSLATION[1])


# name -> (from, to, threshold, seed): the hypotheses and the refit.  Every case passes the honesty condition of
# tests/test_feature_match_host.py (a case that does not is replaced here, never skipped there).
def _ransac_cases():
    cases = {}
    for M in (2, 5, 63, 64, 200):
        for seed in (1, 2):
            p, P, _, _ = ransac_points(M, 100 * M + seed, outliers=0.0 if M == 2 else OUTLIERS)
            cases["m%d_seed%d" % (M, seed)] = (p, P, THRESHOLD, seed)
    p, P, _, _ = ransac_points(200, 31, exact=True)
    cases["m200_exact"] = (p, P, THRESHOLD, 3)
    for scale in (1.05, 1.2):
        p, P, _, _ = ransac_points(200, 41, scale=scale)
        cases["m200_scale_%g" % scale] = (p, P, THRESHOLD, 5)
    p, P, _, _ = ransac_points(64, 51)
    cases["m64_same_from"] = (np.tile(p[:1], (64, 1)), P, THRESHOLD, 1)  # every hypothesis degenerate: NO_MODEL
    p, P, _, _ = ransac_points(200, 61)
    cases["m200_other_seed_a"] = (p, P, THRESHOLD, 11)
    cases["m200_other_seed_b"] = (p, P, THRESHOLD, 12)
    return cases


RANSAC_CASES = _ransac_cases()
SCALE_TOLERANCE = 0.1


def make_set(rng, n, D, ox=None, oy=None, resolution=0.1):
    """n random key points in a 600 x 600 pixel image with random unit descriptors"""
    ox = rng.uniform(-20, 20) if ox is None else ox
    oy = rng.uniform(-20, 20) if oy is None else oy
    return FeatureSet(unit_descriptors(rng, n, D), rng.uniform(0, 600, size=(n, 2)), ox, oy, resolution)


def overlapping_set(rng, query, planted, extra, scale=1.0, theta=THETA, translation=TRANSLATION, outliers=OUTLIERS, noise=NOISE,
                    descriptor_noise=0.05):
    """A set that shares `planted` of the query's features (their descriptors perturbed, their positions the similarity of
    the query's plus noise, a share of them at random positions instead) and has `extra` features of its own, shuffled."""
    D = query.descriptors.shape[1]
    pick = rng.permutation(len(query))[:planted]
    d = query.descriptors[pick].astype(np.float64) + rng.normal(0, descriptor_noise, size=(planted, D))
    d /= np.linalg.norm(d, axis=1)[:, None]
    a, b = similarity(theta, scale)
    ox, oy = rng.uniform(-20, 20, 2)
    world = np.stack([np.float32(query.ox) + query.keypoints[pick, 0].astype(np.float64) * query.resolution,
                      np.float32(query.oy) + query.keypoints[pick, 1].astype(np.float64) * query.resolution], axis=1)
    P = apply(a, b, translation, world) + rng.normal(0, noise, size=(planted, 2))
    out = rng.permutation(planted)[:int(round(outliers * planted))]
    P[out] = rng.uniform(-40, 80, size=(len(out), 2))
    kp = (P - [ox, oy]) / query.resolution
    d = np.concatenate([d, unit_descriptors(rng, extra, D)])
    kp = np.concatenate([kp, rng.uniform(0, 600, size=(extra, 2))])
    order = rng.permutation(len(d))
    return FeatureSet(d[order], kp[order], ox, oy, query.resolution)


def match_scene(D=64, seed=3):
    """Eight stored sets -> (sets, query index, train indices): sets of 0 and 1 key points, one without overlap, three with
    planted overlaps (scale 1 with more than 63 good matches, scale 1.05 with fewer, scale 1.2), a small stranger whose size
    sits behind a chunk of the nearest-neighbour kernel, and the query."""
    rng = np.random.RandomState(seed)
    query = make_set(rng, 300, D)
    sets = [FeatureSet(np.zeros((0, D)), np.zeros((0, 2)), 1.0, 2.0, 0.1),
            make_set(rng, 1, D),
            make_set(rng, 260, D),
            overlapping_set(rng, query, 120, 200),
            overlapping_set(rng, query, 40, 100, scale=1.05),
            overlapping_set(rng, query, 120, 150, scale=1.2),
            make_set(rng, CHUNK + 1, D),
            query]
    return sets, 7, [0, 1, 2, 3, 4, 5, 6]


def capacity_scene(D=16, seed=4):
    """A query of MAX_GOOD + 4 features against a copy of itself under the planted similarity (every match good: above the
    capacity) and against a set with a planted overlap (unaffected) -> (sets, query index, train indices)"""
    rng = np.random.RandomState(seed)
    query = make_set(rng, MAX_GOOD + 4, D)
    copy = overlapping_set(rng, query, len(query), 0, outliers=0.0, descriptor_noise=0.0)
    return [copy, overlapping_set(rng, query, 80, 60, descriptor_noise=0.01), query], 2, [0, 1]


# name -> (sets, query, train, Options)
def _match_cases():
    s, q, t = match_scene()
    c, cq, ct = capacity_scene()
    rng = np.random.RandomState(5)
    same = make_set(rng, 90, 64)
    same.keypoints[:] = same.keypoints[0]  # every `from` point equal: every hypothesis degenerate
    return {"scene": (s, q, t, Options()), "scene_from_overlap": (s, 3, [7, 2, 5, 0], Options(seed=8)),
            "capacity": (c, cq, ct, Options()), "same_keypoints": ([overlapping_set(rng, same, 70, 30), same], 1, [0], Options())}


MATCH_CASES = _match_cases()
