"""The trajectory buffer and the CPU model of the batch assembler, without a device: the reference's own known answers
(transform/transform_interpolation_buffer_test.cc), dliom_trajectory_lookup against the model in bits, and the refusals
that are decided before a device is touched."""
import numpy as np
import pytest

import assemble_common as ac
import dliom
from dliom import synth


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    directory = tmp_path_factory.mktemp("assemble_model")
    return ac.build_model(directory), directory


IDENTITY = ac.IDENTITY
# Rigid3d::Translation(10, 10, 10) * Rigid3d::Rotation(AngleAxisd(2., UnitZ()))
TURNED = np.concatenate([[10.0, 10.0, 10.0], synth.quat_from_axis_angle((0.0, 0.0, 1.0), 2.0)])


def both(model, times, poses, at):
    """Has / Lookup of the model and of dliom_trajectory_lookup for the times `at`; asserts that they agree in bits."""
    exe, directory = model
    pushed, results = ac.run_model(exe, times, poses, [ac.lookup_op(at)], directory)
    assert pushed == 0
    has, want = results[0]
    trajectory = dliom.Trajectory(None, times, poses)
    for k, t in enumerate(at):
        assert trajectory.has(t) == bool(has[k]), t
        got = trajectory.lookup(t)
        if has[k]:
            assert got.tobytes() == want[k].tobytes(), (t, got, want[k])
        else:
            assert got is None
    trajectory.close()
    return has, want


def test_has_known_answers(model):
    assert list(both(model, [], np.zeros((0, 7)), [50])[0]) == [False]
    assert list(both(model, [50], [IDENTITY], [25, 50, 75])[0]) == [False, True, False]
    assert list(both(model, [50, 100], [IDENTITY, IDENTITY], [25, 50, 75, 100, 125])[0]) == [False, True, True, True, False]


def test_lookup_known_answers(model):
    has, pose = both(model, [50, 100], [IDENTITY, TURNED], [75])
    want = np.concatenate([[5.0, 5.0, 5.0], synth.quat_from_axis_angle((0.0, 0.0, 1.0), 1.0)])
    assert has[0] and np.max(np.abs(pose[0] - want)) <= 1e-6  # IsNearly(..., 1e-6)
    has, pose = both(model, [75], [IDENTITY], [75])
    assert has[0] and np.max(np.abs(pose[0] - IDENTITY)) <= 1e-6


def test_lookup_equals_model_in_bits(model):
    rng = np.random.RandomState(11)
    n = 37
    times = ac.EPOCH + np.cumsum(rng.randint(1, 400_000, size=n)).astype(np.int64)
    poses = np.array([np.concatenate([rng.uniform(-20.0, 20.0, size=3), ac.random_quaternion(rng)]) for _ in range(n)])
    for i in range(1, n):  # neighbours a few degrees apart, as on a trajectory
        step = synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.01, 0.1))
        poses[i, 3:] = synth.quat_mul(poses[i - 1, 3:], step)
    poses[9, 3:] = -poses[9, 3:]  # the intervals into and out of node 9 have d < 0
    poses[19, 3:] = poses[20, 3:] = [0.5, 0.5, -0.5, 0.5]  # identical rotations, d = 1 exactly: the absD >= one branch
    times[30] = times[29]  # duplicated node times: lower_bound finds the first
    times[31] = times[29]
    mid = (times[:-1] + times[1:]) // 2
    at = np.concatenate([times, mid - 1, mid, mid + 1, [times[0] - 1, times[-1] + 1]])
    has, pose = both(model, times, poses, at)
    assert np.count_nonzero(has) == len(at) - 2
    d = np.sum(poses[8, 3:] * poses[9, 3:])
    assert d < 0.0 and np.sum(poses[19, 3:] * poses[20, 3:]) >= 1.0 - 2.220446049250313e-16


def test_model_counts_branches_and_intervals(model):
    """The drives are honest on the CPU before a device sees them."""
    exe, directory = model
    for nodes in (2, 3, 37, 200):
        times, poses, cloud_time, xyzt = ac.drive(16, 256, nodes)
        pushed, results = ac.run_model(exe, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, xyzt)], directory)
        assert pushed == 0
        kept = ac.honest(results[0], nodes)
        assert (kept < len(xyzt)) == (nodes <= 3)  # the short trajectories are overhung at both ends


def test_refusals_without_a_device(model):
    exe, directory = model
    pushed, _ = ac.run_model(exe, [50, 100, 99], [IDENTITY] * 3, [], directory)
    assert pushed == -1
    with pytest.raises(dliom.DliomError) as e:
        dliom.Trajectory(None, [50, 100, 99], [IDENTITY] * 3)
    assert e.value.status == dliom.ERR_INVALID_ARGUMENT
    dliom.Trajectory(None, [50, 50, 100], [IDENTITY] * 3).close()  # equal neighbours are allowed
    L = dliom.load_library()
    import ctypes as C
    h = C.c_void_p()
    t, p = np.array([50], dtype=np.int64), np.array(IDENTITY)
    tp, pp = t.ctypes.data_as(C.POINTER(C.c_int64)), p.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dliom_trajectory_create(None, tp, pp, 1, None) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_create(None, None, pp, 1, C.byref(h)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_create(None, tp, None, 1, C.byref(h)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_create(None, tp, pp, -1, C.byref(h)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_lookup(None, 50, C.byref(C.c_int()), None) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_destroy(None) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_assemble_check_stats(None, None, None, None, None) == dliom.ERR_INVALID_ARGUMENT
    # a host-only trajectory cannot be assembled against (no context), and NULL arguments are refused first
    assert L.dliom_trajectory_create(None, tp, pp, 1, C.byref(h)) == dliom.OK
    kept, origin = C.c_int64(), np.zeros(3, dtype=np.float32)
    out = C.c_void_p()
    assert L.dliom_cloud_from_sensor_points(None, h, 50, None, 0, pp, C.byref(out), origin.ctypes.data_as(C.POINTER(C.c_float)), None,
                                            0, C.byref(kept)) == dliom.ERR_INVALID_ARGUMENT
    assert L.dliom_trajectory_destroy(h) == dliom.OK
