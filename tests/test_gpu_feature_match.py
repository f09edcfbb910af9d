"""Submap feature matching on the device (d-liom_amd/csrc/feature_match.hip) against the CPU model
(tests/cpp/feature_match_model.cc), bit for bit: the nearest neighbours on the edges of the kernel's tile and chunk, the
hypotheses and the refit, whole match calls, and the C++ adapter."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_match_common as fc  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = fc.CHUNK


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
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("feature_match_model")
    return fc.build_model(d), d


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def device_knn(dl, ctx, q, t):
    index = dl.FeatureIndex(ctx, q.shape[1])
    try:
        index.add(1, q, np.zeros((len(q), 2)), 0.0, 0.0, 0.1)
        index.add(2, t, np.zeros((len(t), 2)), 0.0, 0.0, 0.1)
        return index.knn(1, 2, len(q))
    finally:
        index.close()


def assert_knn_equal(got, want):
    for g, w, name in zip(got, want, ("j0", "j1", "d0", "d1")):
        same = np.array_equal(g, w) if g.dtype == np.int32 else np.array_equal(bits(g), bits(w))
        assert same, (name, np.flatnonzero(g != w)[:8])


@pytest.mark.parametrize("D", [4, 64, 128])
def test_knn_sizes(dl, ctx, model, D):
    """Every nq on the edges of a wave and of the 256-query tile against every nt on the edges of the LDS chunk: one index
    holds the sets, the model's answers are computed once a pair."""
    exe, d = model
    rng = np.random.RandomState(D)
    queries = {n: fc.unit_descriptors(rng, n, D) for n in (2, 63, 64, 65, 130, 257)}
    trains = {n: fc.unit_descriptors(rng, n, D) for n in (2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)}
    index = dl.FeatureIndex(ctx, D)
    try:
        for n, q in queries.items():
            index.add(n, q, np.zeros((n, 2)), 0.0, 0.0, 0.1)
        for n, t in trains.items():
            index.add(1000 + n, t, np.zeros((n, 2)), 0.0, 0.0, 0.1)
        for nq, q in queries.items():
            for nt, t in trains.items():
                assert_knn_equal(index.knn(nq, 1000 + nt, nq), fc.model_knn(exe, d, q, t))
    finally:
        index.close()


def test_knn_other_descriptor_sizes(dl, ctx, model):
    """Sizes that are no power of two run a kernel padded with zeros: 8, 20, 36, 100."""
    exe, d = model
    for D in (8, 20, 36, 100):
        rng = np.random.RandomState(D)
        q, t = fc.unit_descriptors(rng, 70, D), fc.unit_descriptors(rng, CHUNK + 3, D)
        assert_knn_equal(device_knn(dl, ctx, q, t), fc.model_knn(exe, d, q, t))


def test_knn_duplicates_and_self(dl, ctx, model):
    """A train set with duplicated descriptors: the lowest index wins, and d0 == d1 fails the ratio test.  The query set as
    its own train set: every query finds itself at distance 0."""
    exe, d = model
    rng = np.random.RandomState(9)
    t = fc.unit_descriptors(rng, 40, 64)
    t = np.concatenate([t, t[:20], t[10:30]])  # rows 0..19 twice, 10..19 three times, beyond the first chunk as well
    q = np.concatenate([t[:30] + np.float32(0.01), fc.unit_descriptors(rng, 10, 64)])
    got, want = device_knn(dl, ctx, q, t), fc.model_knn(exe, d, q, t)
    assert_knn_equal(got, want)
    j0, j1, d0, d1 = got
    assert np.array_equal(j0[:20], np.arange(20)) and np.array_equal(j1[:20], 40 + np.arange(20))
    assert np.array_equal(j1[10:20], 40 + np.arange(10, 20)) and np.array_equal(bits(d0[:20]), bits(d1[:20]))
    # a pair of sets whose every nearest pair is a duplicate has no good match, whatever the ratio below 1
    index = dl.FeatureIndex(ctx, 64)
    try:
        index.add(1, q[:20], rng.uniform(0, 600, (20, 2)), 0.0, 0.0, 0.1)
        index.add(2, t, rng.uniform(0, 600, (len(t), 2)), 0.0, 0.0, 0.1)
        results, _ = index.match(1, [2], dl.feature_match_options(0.999999, 1, 3.0, 0.1))
        assert results["status"][0] == fc.TOO_FEW_GOOD_MATCHES and results["good_matches"][0] == 0
    finally:
        index.close()
    got, want = device_knn(dl, ctx, t[:40], t[:40]), fc.model_knn(exe, d, t[:40], t[:40])
    assert_knn_equal(got, want)
    assert np.array_equal(got[0], np.arange(40)) and not got[2].any() and got[3].all()


@pytest.mark.parametrize("name", list(fc.RANSAC_CASES))
def test_ransac(dl, ctx, model, name):
    """Status, hypothesis index, inlier mask and the bits of a, b, tx, ty (and of scale and theta, made on the host)."""
    exe, d = model
    p, P, threshold, seed = fc.RANSAC_CASES[name]
    want, want_mask, _ = fc.model_ransac(exe, d, p, P, threshold, seed)
    got, mask = dl.feature_ransac(ctx, p, P, threshold, seed)
    print(name, got)
    for k in ("status", "inliers", "hypothesis", "num_hypotheses"):
        assert got[k] == want[k], k
    assert np.array_equal(mask, want_mask)
    for k in ("a", "b", "tx", "ty", "scale", "theta"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
    if name == "m64_same_from":
        assert got["status"] == fc.NO_MODEL
    if name.startswith("m200_scale"):
        assert (abs(got["scale"] - 1) > fc.SCALE_TOLERANCE) == name.endswith("1.2")


def test_ransac_two_seeds(dl, ctx):
    a = dl.feature_ransac(ctx, *fc.RANSAC_CASES["m200_other_seed_a"])[0]
    b = dl.feature_ransac(ctx, *fc.RANSAC_CASES["m200_other_seed_b"])[0]
    assert a["status"] == b["status"] == fc.MATCHED and a["hypothesis"] != b["hypothesis"]


def fill(index, sets, first_key=100):
    for k, s in enumerate(sets):
        index.add(first_key + k, s.descriptors, s.keypoints, s.ox, s.oy, s.resolution)


def assert_results_equal(got, want, first_key=100):
    assert np.array_equal(got["key"], want["key"] + first_key)
    for k in fc.SUBMAP_MATCH.names[1:]:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


@pytest.mark.parametrize("name", ["scene", "scene_from_overlap", "same_keypoints"])
def test_match(dl, ctx, model, name):
    """Every field of every result equals the model's; a second call gives the same bytes; one read-back a call."""
    exe, d = model
    sets, query, train, options = fc.MATCH_CASES[name]
    want = fc.model_match(exe, d, sets, query, train, options)[0]
    index = dl.FeatureIndex(ctx, sets[query].descriptors.shape[1])
    try:
        fill(index, sets)
        assert len(index) == len(sets) and index.memory_stats()["keypoints"] == sum(len(s) for s in sets)
        keys = [100 + t for t in train]
        before = ctx.read_backs()
        got, stats = index.match(100 + query, keys, options.device(dl))
        assert ctx.read_backs() - before == 1 == stats["read_backs"]
        print(name, got, stats)
        assert_results_equal(got, want)
        assert stats["pairs"] == len(train) and stats["matched"] == int((want["status"] == fc.MATCHED).sum())
        assert stats["too_few_keypoints"] == int((want["status"] == fc.TOO_FEW_KEYPOINTS).sum())
        again, _ = index.match(100 + query, keys, options.device(dl))
        assert again.tobytes() == got.tobytes()
    finally:
        index.close()


def test_match_remove_and_refusals(dl, ctx, model):
    """After remove, the key is refused and the others are unchanged; malformed input fails the whole call."""
    exe, d = model
    sets, query, train, options = fc.MATCH_CASES["scene"]
    want = fc.model_match(exe, d, sets, query, train, options)[0]
    index = dl.FeatureIndex(ctx, 64)
    try:
        fill(index, sets)
        o = options.device(dl)
        index.remove(100 + 2)
        assert len(index) == len(sets) - 1
        for call in (lambda: index.match(100 + query, [100 + t for t in train], o), lambda: index.remove(100 + 2),
                     lambda: index.match(100 + 2, [100], o), lambda: index.add(100, sets[3].descriptors, sets[3].keypoints, 0, 0, 0.1),
                     lambda: index.add(500, np.full((2, 64), np.nan), np.zeros((2, 2)), 0, 0, 0.1),
                     lambda: index.add(500, np.zeros((2, 64)), np.zeros((2, 2)), np.inf, 0, 0.1),
                     lambda: index.match(100 + query, [103], dl.feature_match_options(np.nan, 10, 3.0, 0.1))):
            with pytest.raises(dl.DliomError) as e:
                call()
            assert e.value.status == dl.ERR_INVALID_ARGUMENT
        assert len(index) == len(sets) - 1
        kept = [t for t in train if t != 2]
        got, _ = index.match(100 + query, [100 + t for t in kept], o)
        assert_results_equal(got, want[[train.index(t) for t in kept]])
        none, stats = index.match(100 + query, [], o)
        assert len(none) == 0 and stats["read_backs"] == 0
    finally:
        index.close()


def test_match_capacity(dl, ctx, model):
    """One pair above DLIOM_FEATURE_MAX_GOOD good matches reports capacity for that pair; the other is right."""
    exe, d = model
    sets, query, train, options = fc.MATCH_CASES["capacity"]
    want = fc.model_match(exe, d, sets, query, train, options)[0]
    index = dl.FeatureIndex(ctx, sets[query].descriptors.shape[1])
    try:
        fill(index, sets)
        got, stats = index.match(100 + query, [100 + t for t in train], options.device(dl))
        assert_results_equal(got, want)
        assert list(got["status"]) == [dl.ERR_CAPACITY, fc.MATCHED] and got["good_matches"][0] == fc.MAX_GOOD + 4
        assert stats["over_capacity"] == 1 and stats["matched"] == 1
    finally:
        index.close()


def test_adapter(dl, model, tmp_path):
    """mapping::constraints::SubmapFeatureMatcher (tests/cpp/feature_match_adapter.cc) over the scene: the adjacency rule
    (same trajectory within two submap indices is not searched), and the returned Rigid3d's against Embed3D of the model's
    result -- translation (tx, ty, 0) exactly, rotation (cos(theta / 2), 0, 0, sin(theta / 2)) to 4e-16: two libraries'
    cos and sin of one double, each within an ulp of a value below 1."""
    exe, d = model
    sets, query, train, options = fc.MATCH_CASES["scene"]
    want = fc.model_match(exe, d, sets, query, train, options)[0]
    assert want["status"][3] == want["status"][4] == fc.MATCHED
    adapter = str(tmp_path / "feature_match_adapter")
    libdir = os.path.dirname(dl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(fc.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", adapter, os.path.join(fc.ROOT, "tests", "cpp", "feature_match_adapter.cc"),
                           dl.LIB_PATH, "-Wl,-rpath," + libdir])
    # set 3 (matched) is on another trajectory at a near index: searched; set 4 (matched) is the query's neighbour: not
    ids = [(0, 0), (0, 1), (0, 2), (1, 9), (0, 8), (0, 5), (0, 6), (0, 10)]
    src, dst = os.path.join(str(d), "fm_in.bin"), str(tmp_path / "adapter.bin")
    fc.model_match(exe, d, sets, query, train, options)  # leaves its input file behind
    subprocess.check_call([adapter, src, dst] + [str(v) for pair in ids for v in pair])
    data = open(dst, "rb").read()

    def read(at):
        n = np.frombuffer(data, "<i4", 1, at)[0]
        rec = np.frombuffer(data, np.dtype([("id", "<i4", 2), ("pose", "<f8", 7)]), n, at + 4)
        return {tuple(r["id"]): r["pose"] for r in rec}, at + 4 + 64 * n
    first, at = read(0)
    second, at = read(at)
    assert at == len(data)
    assert sorted(first) == [(1, 9)]
    for matched, k in ((first[(1, 9)], 3),):
        theta = want["theta"][k]
        assert matched[:3].tobytes() == np.array([want["tx"][k], want["ty"][k], 0.0]).tobytes()
        assert np.abs(matched[3:] - [np.cos(0.5 * theta), 0.0, 0.0, np.sin(0.5 * theta)]).max() <= 4e-16
    # (1, 9) deleted, the query's features again as (99, 0): its old neighbour (0, 8) is searched now, (1, 9) is gone
    assert sorted(second) == [(0, 8)]
    assert second[(0, 8)][:3].tobytes() == np.array([want["tx"][4], want["ty"][4], 0.0]).tobytes()
