"""The approximate voxel grid without a GPU: the parallel restatement the device runs against the sequential loop of the
definition (tests/approx_voxel_common.py), that loop against the model the NDT tests already use, and the new names and
argument checks of the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_voxel_common as av  # noqa: E402
import ndt_common as nd  # noqa: E402


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.mark.parametrize("scale", [0.3, 3.0, 30.0])
def test_parallel_equals_sequential_on_random_clouds(scale):
    """Ten clouds a scale, every third clustered; at 0.3 m a few voxels hold everything, at 30 m the slots churn"""
    for trial in range(10):
        cloud = av.random_cloud(1500 + 37 * trial, seed=100 * trial + int(10 * scale), scale=scale, clustered=trial % 3 == 2)
        for leaf in (0.2, 0.3):
            want = av.sequential(cloud, leaf)
            assert av.same(av.parallel(cloud, leaf), want), (scale, trial, leaf)
            assert 0 < len(want) <= len(cloud)


def test_parallel_equals_sequential_on_the_made_cases():
    cases = {"alternating": av.alternating(), "a-b-a": av.a_b_a(), "every-slot": av.every_slot(), "one-voxel": av.one_voxel(),
             "faces-0.2": av.faces(0.2), "wrapping": av.wrapping(), "one": av.random_cloud(1, 1), "two": av.random_cloud(2, 2)}
    for name, cloud in cases.items():
        assert av.same(av.parallel(cloud, 0.2), av.sequential(cloud, 0.2)), name
    assert av.same(av.parallel(av.faces(0.3), 0.3), av.sequential(av.faces(0.3), 0.3))
    assert len(av.parallel(np.zeros((0, 3), np.float32), 0.2)) == 0


def test_the_made_cases_are_what_they_claim():
    assert len(av.sequential(av.alternating(100), 0.2)) == 100  # every point evicts
    _, v, slot = av.voxels_and_slots(av.alternating(100), 0.2)
    assert len(set(slot)) == 1 and len({tuple(r) for r in v}) == 2
    aba = av.sequential(av.a_b_a(), 0.2)
    _, v, slot = av.voxels_and_slots(av.a_b_a(), 0.2)
    assert len(aba) == 3 and len(set(slot)) == 1 and len({tuple(r) for r in v}) == 2  # A is emitted twice
    _, _, slot = av.voxels_and_slots(av.every_slot(), 0.2)
    assert len(set(slot)) == av.SLOTS and len(av.sequential(av.every_slot(), 0.2)) == av.SLOTS
    assert len(av.sequential(av.one_voxel(), 0.2)) == 1
    _, v, _ = av.voxels_and_slots(av.wrapping(), 0.2)
    assert np.abs(v).min() > 2 ** 30 - 4096 and (np.abs(v * 7171) > 2 ** 32).all()


def test_sequential_equals_the_ndt_tests_model():
    """Two independent writings of the loop"""
    for cloud in (av.random_cloud(700, 5, 3.0), av.a_b_a(), av.faces(0.2)):
        assert av.same(av.sequential(cloud, 0.2), nd.approximate_voxel_grid(cloud, 0.2))


def test_the_model_refuses_what_the_definition_refuses():
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, 5e8]):  # 5e8 / 0.2 is beyond int32
        with pytest.raises(ValueError):
            av.sequential(np.array([bad], np.float32), 0.2)


def test_argument_checks_without_a_device(dl):
    L = dl.load_library()
    h = C.c_void_p()
    o = dl.ndt_options()
    assert L.dliom_cloud_approximate_voxel_filter(None, None, C.c_float(0.2), C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_timed_cloud_points(None, None, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_scan_matcher_create(None, C.byref(o), C.c_float(0.2), C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ndt_scan_matcher_match(None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    v = C.c_int()
    assert L.dliom_ndt_scan_matcher_has_target(None, C.byref(v)) == dl.ERR_INVALID_ARGUMENT
    L.dliom_ndt_scan_matcher_destroy(None)  # like the other destroyers: nothing happens
