"""The inputs of tests/test_gpu_cloud_bounds.py under the CPU models alone (no GPU): every prescribed cloud keeps and
loses the points it was built to keep and lose -- by the oracle's voxel filters, tests/cpp/outlier_model.cc,
tests/cpp/points_batch_model.cc and tests/cpp/assemble_model.cc -- and every case that claims to remove the farthest
input point does; ref_max_norm equals a plain loop; dliom_cloud_bounds is declared and refuses null arguments."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_common as ac  # noqa: E402
import cloud_bounds_common as cb  # noqa: E402
import outlier_common as oc  # noqa: E402
import points_batch_common as pb  # noqa: E402
from cloud_bounds_common import f32  # noqa: E402


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def test_symbol_is_declared_and_refuses_null(dl):
    assert ("dliom_cloud_bounds", C.c_int, [dl._vp, dl._f32p, dl._f32p]) in dl.SYMBOLS
    assert "int dliom_cloud_bounds(const dliom_cloud* cloud, float* max_norm, float abs_max[3]);" in open(
        os.path.join(oc.ROOT, "include", "dliom.h")).read()
    assert hasattr(dl.PointCloud, "bounds")
    L = dl.load_library()
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # stands for a cloud; never dereferenced by a refusal
    m, a = C.c_float(), (C.c_float * 3)()
    assert L.dliom_cloud_bounds(None, C.byref(m), a) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_bounds(fake, None, a) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_bounds(fake, C.byref(m), None) == dl.ERR_INVALID_ARGUMENT


def test_reference_equals_a_plain_loop():
    rng = np.random.RandomState(1)
    pts = (rng.normal(size=(300, 3)) * rng.uniform(0, 30, (300, 1))).astype(f32)
    assert cb.bits(cb.ref_max_norm(pts)) == cb.bits(cb.ref_max_norm_loop(pts))
    assert cb.ref_max_norm(pts) == f32(np.sqrt(np.max((pts[:, 0] * pts[:, 0] + (pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2])))))
    for case in cb.cases("range", 257) + cb.sampler_cases()[-6:]:
        for p in (case.points, case.points[case.keep]):
            assert cb.bits(cb.ref_max_norm(p)) == cb.bits(cb.ref_max_norm_loop(p)), case.name
    nan, inf = np.nan, np.inf
    assert cb.bits(cb.ref_max_norm(np.zeros((0, 3)))) == cb.bits(0.0)
    assert cb.bits(cb.ref_max_norm([[-0.0, 0.0, -0.0]])) == cb.bits(0.0)  # +0, not -0
    assert cb.bits(cb.ref_max_norm([[nan, 0, 0], [3, 4, 0], [1e30, nan, 1]])) == cb.bits(5.0)  # a NaN never wins
    assert cb.ref_max_norm([[3, 4, 0], [1, -inf, 0]]) == f32(inf)  # +inf does
    assert cb.ref_max_norm([[inf, nan, 0], [3, 4, 0]]) == f32(5.0)
    tiny = cb.ref_max_norm([[1.5e-20, -1.2e-20, 0.7e-20]])
    assert 0 < tiny * tiny < np.finfo(f32).tiny  # a denormal squared norm


@pytest.mark.parametrize("n", cb.SIZES)
def test_range_cases_keep_what_they_claim(n):
    for case in cb.cases("range", n):
        assert np.array_equal(cb.range_keep(case.points, case.params), case.keep), case.name
        cb.premise(case)


def test_range_value_edges_are_what_they_claim():
    names = [c.name for c in cb.cases("range", 257)]
    assert len(names) == len(set(names))
    for want in ("tie", "origin", "denormal", "nothing_kept", "kept_inf"):
        assert "range_" + want in names
    by = {c.name: c for c in cb.cases("range", 257)}
    tie = by["range_tie"]
    assert cb.ref_max_norm(tie.points[tie.keep]) == f32(np.sqrt(f32(tie.points[64, 0] ** 2 + (tie.points[64, 1] ** 2 + tie.points[64, 2] ** 2))))
    assert tie.points[200].tobytes() == (-tie.points[64]).tobytes() and tie.keep[64] and tie.keep[200]
    assert cb.bits(cb.ref_max_norm(by["range_origin"].points[by["range_origin"].keep])) == cb.bits(0.0)
    assert np.signbit(by["range_origin"].points[by["range_origin"].keep]).any()
    d = cb.ref_max_norm(by["range_denormal"].points[by["range_denormal"].keep])
    assert 0 < d * d < np.finfo(f32).tiny
    assert cb.ref_max_norm(by["range_kept_inf"].points[by["range_kept_inf"].keep]) == f32(np.inf)
    assert not by["range_nothing_kept"].keep.any()


def test_range_cases_equal_the_model(tmp_path):
    model = oc.build_model(tmp_path)
    all_cases = [c for n in cb.SIZES for c in cb.cases("range", n)]
    results, _ = oc.run_model(model, 0.5, [oc.op(oc.RANGE, c.points, (0, 0, 0), *c.params) for c in all_cases], tmp_path)
    for case, (status, index) in zip(all_cases, results):
        assert status == 0 and np.array_equal(index, np.flatnonzero(case.keep)), case.name


def test_remover_cases_equal_the_model(tmp_path):
    """Hits in the voxels of the points to keep, no rays: a voxel with a hit keeps its points (0 < 3 hits), one without
    removes them (!(0 < 0))."""
    model = oc.build_model(tmp_path)
    for n in cb.SIZES:
        for case in cb.cases("remover", n):
            results, _ = oc.run_model(model, cb.EDGE, [oc.op(oc.MARK, case.points[case.keep]), oc.op(oc.FILTER, case.points)], tmp_path)
            assert results[0] == 0 and results[1][0] == 0 and np.array_equal(results[1][1], np.flatnonzero(case.keep)), case.name
            cb.premise(case)


@pytest.mark.parametrize("n", cb.SIZES)
def test_voxel_cases_equal_the_oracle(orc, n):
    for case in cb.cases("voxel", n):
        keep = np.flatnonzero(case.keep)
        if len(case.points):
            assert np.array_equal(orc.voxel_filter(cb.EDGE, case.points), keep), case.name
            want = orc.adaptive_voxel_filter(*cb.ADAPTIVE_ALL, case.points)
            assert want.tobytes() == case.points[keep].tobytes(), case.name
        cb.premise(case)
        if "kept_far" in case.name:  # the cropped filter removes the farthest point before it filters: beyond max_range
            cropped = orc.adaptive_voxel_filter(*cb.ADAPTIVE_CROPPED, case.points)
            assert cb.ref_max_norm(case.points) > cb.ref_max_norm(cropped) > 0 or n == 1, case.name


def test_sampler_cases_equal_the_model(tmp_path):
    model = pb.build_model(tmp_path)
    all_cases = cb.sampler_cases()
    results = pb.run_model(model, [pb.pulse_op(c.params, 0, 0, len(c.points)) for c in all_cases], tmp_path)
    for case, (keep, pulses, samples) in zip(all_cases, results):
        assert np.array_equal(keep, case.keep) and pulses == len(case.points) and samples == case.keep.sum(), case.name
        kept, everything = cb.premise(case)
        if "removed_far" in case.name:
            assert everything > kept
    names = [c.name for c in all_cases]
    assert len(names) == len(set(names))
    # the repaired case: the farthest point is one the wrong first pass DROPS and the sequential loop keeps.  (The other
    # way round -- kept by the first pass, dropped in the end -- does not exist for 0.55 from (0, 0) over 4097 pulses:
    # every wrong guess is one too high.)
    repaired = [c for c in all_cases if c.name.startswith("sampler_0.55_repaired_kept_far")]
    assert len(repaired) == 1
    case = repaired[0]
    far = int(case.name.rsplit("_", 1)[1])
    first = cb.sampler_first_pass_keep(0.55, 4097)
    assert not np.any(first & ~case.keep)
    s = (case.points[case.keep].astype(np.float64) ** 2).sum(axis=1)
    assert case.keep[far] and not first[far] and int(np.flatnonzero(case.keep)[np.argmax(s)]) == far
    assert cb.ref_max_norm(case.points[first]) < cb.ref_max_norm(case.points[case.keep])  # the first pass's bound is too small
    wrong_chunks = {int(i) // cb.CHUNK for i in np.flatnonzero(first != case.keep)}
    assert {1600 // 64, 2880 // 64, 3200 // 64} <= wrong_chunks, sorted(wrong_chunks)
    assert np.array_equal(cb.sampler_first_pass_keep(0.5, 4097), cb.sampler_keep(0.5, 4097))  # 0.5: no repair
    by = {c.name: c for c in all_cases}
    assert cb.ref_max_norm(by["sampler_kept_inf"].points[by["sampler_kept_inf"].keep]) == f32(np.inf)
    nan = by["sampler_kept_nan"]
    assert np.isnan(nan.points[nan.keep]).any()
    assert np.isfinite(cb.ref_max_norm(nan.points[nan.keep])) and cb.ref_max_norm(nan.points[nan.keep]) > 14.9
    assert cb.bits(cb.ref_max_norm(by["sampler_origin"].points[by["sampler_origin"].keep])) == cb.bits(0.0)


@pytest.mark.parametrize("n", cb.SIZES)
def test_frontend_cases_equal_the_oracle(orc, n):
    """The oracle's AddRangeData keeps exactly the ranges a case claims, in their order, so the farthest return sits at the
    case's place in the returns cloud.  A range "removed_far" by the gate lies farther out than every return.  A
    "voxel_removed" one is dropped by the first voxel filter, not by the gate, and -- the frames of input and output
    differ by the scan's motion, more than its 2 cm -- the premise is taken in the output's frame: without the earlier
    point of its voxel it is a return, and the bound is larger."""
    seen = set()
    for case in cb.frontend_cases(n):
        returns, index = cb.frontend_oracle(orc, case)
        keep = np.flatnonzero(case.keep)
        assert np.array_equal(index, keep) and len(returns) == len(keep), case.name
        bound = cb.ref_max_norm(returns)
        xyz = case.points[:, :3]
        s = (returns.astype(np.float64) ** 2).sum(axis=1)
        kind = "voxel" if "_voxel_" in case.name else "general" if "general_path" in case.name else "plain"
        far = int(case.name.rsplit("_", 1)[1]) if case.name[-1].isdigit() else None
        if "kept_far" in case.name or "only_kept" in case.name:
            assert keep[int(np.argmax(s))] == far and (len(s) == 1 or np.sort(s)[-2] < s.max()), case.name
            seen.add((kind, "kept"))
        if "removed_far" in case.name:
            assert not case.keep[far], case.name
            voxels = orc.voxel_filter(0.5 * f32(cb.FRONTEND_VFS), xyz)
            r = np.sqrt((xyz[far].astype(np.float64) ** 2).sum())
            if kind == "voxel":
                assert far not in voxels and r < case.params[1] - 1.0, case.name  # not the gate's doing
                earlier = int(np.flatnonzero(case.keep[:far])[-1])
                without, index = cb.frontend_oracle(orc, case, np.delete(case.points, earlier, axis=0))
                assert far - 1 in index and cb.ref_max_norm(without) > bound, case.name
            else:
                assert far in voxels and r > case.params[1] + 10.0, case.name  # the gate's
                assert cb.ref_max_norm(xyz) > bound + f32(10.0), case.name
            seen.add((kind, "removed"))
        if kind == "general":  # beyond 4095 edges of the second, coarser filter in input and output
            assert np.abs(xyz[case.keep]).max() > 4096 * cb.FRONTEND_VFS and np.abs(returns).max() > 4096 * cb.FRONTEND_VFS, case.name
        elif len(returns):
            assert np.abs(xyz).max() < 4095 * 0.5 * cb.FRONTEND_VFS and np.abs(returns).max() < 4000 * cb.FRONTEND_VFS, case.name
        if case.name == "frontend_nothing_kept":
            assert len(returns) == 0 and bound == 0
            seen.add("nothing")
    want = {("plain", "kept"), ("plain", "removed")}
    if n > 1:
        want |= {("voxel", "removed")}
    if n == 257:
        want |= {("general", "kept"), ("general", "removed"), "nothing"}
    assert seen == want, (n, seen)


def test_assemble_cases_equal_the_model(tmp_path):
    model = ac.build_model(tmp_path)
    times, poses, cloud_time = cb.assemble_trajectory()
    all_cases = cb.assemble_cases()
    pushed, results = ac.run_model(model, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, c.points) for c in all_cases], tmp_path)
    assert pushed == 0
    for case, r in zip(all_cases, results):
        assert r["status"] == 0 and np.array_equal(r["index"], np.flatnonzero(case.keep)), case.name
        bound = cb.ref_max_norm(r["xyz"])
        if "kept_far" in case.name or "only_kept" in case.name:  # the farthest map-frame point is the one put far out
            far = int(case.name.rsplit("_", 1)[1])
            s = (r["xyz"].astype(np.float64) ** 2).sum(axis=1)
            assert r["index"][int(np.argmax(s))] == far, case.name
        if "removed_far" in case.name:
            assert cb.ref_max_norm(case.points[:, :3]) > bound + f32(50.0), case.name
        if case.name == "assemble_kept_inf":
            # (a rotation mixes the axes: the infinite coordinate comes out as infinities and NaNs, as in the reference)
            assert not np.isfinite(r["xyz"]).all()
        if case.name == "assemble_kept_nan":
            assert np.isnan(r["xyz"]).any() and np.isfinite(bound) and bound > 70.0
