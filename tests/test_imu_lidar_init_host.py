"""The IMU-LiDAR initialisation's arithmetic (csrc/imu_lidar_init.cc, no GPU): dliom_imu_static_initialization against the
numpy model of its statement (tests/imu_lidar_init_common.py) bit for bit, the model against a rotation built independently
with scipy, the written rule for nearly opposite vectors, the refusals, and the same file under the host sanitizers in a
stand-alone program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imu_lidar_init_common as il  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.80511
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def tilted_samples(n, roll, pitch, seed):
    """A platform at rest, tilted: the accelerometer reads R^T (0, 0, g) plus a bias and noise, the gyroscope its bias and
    noise"""
    rng = np.random.RandomState(seed)
    tilt = Rotation.from_euler("xyz", [roll, pitch, 0.3])
    acc = tilt.inv().apply([0.0, 0.0, G]) + np.array([0.02, -0.01, 0.03]) + 0.05 * rng.standard_normal((n, 3))
    gyr = np.array([1e-3, -2e-3, 5e-4]) + 1e-3 * rng.standard_normal((n, 3))
    return acc, gyr


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


@pytest.mark.parametrize("n,roll,pitch", [(1, 0.0, 0.0), (8, 0.2, -0.1), (1600, -0.7, 0.4), (333, 2.5, 0.1)])
def test_static_initialization_equals_the_model_bit_for_bit(dl, n, roll, pitch):
    acc, gyr = tilted_samples(n, roll, pitch, seed=n)
    got, want = dl.imu_static_initialization(acc, gyr, G), il.static_initialization(acc, gyr, G)
    assert not want["opposite"]
    for key in ("R", "ba", "bg", "P", "V"):
        assert same_bits(got[key], want[key]), (key, got[key], want[key])
    assert not got["P"].any() and not got["V"].any()


def test_static_initialization_on_a_tilted_mean_against_scipy(dl):
    """R built independently: the rotation about (mean x up) / |mean x up| by the angle between the two, scipy's rotation
    vector.  The bound: the model forms R's entries from about 25 rounded operations on numbers of size <= 2 (two
    normalisations, a dot, a cross, sqrt, a reciprocal, the matrix's products), scipy's about as many from sin, cos and
    arccos, each within an ulp or so; arccos near a tilt of 0.76 rad magnifies nothing.  64 * 2^-52 an entry covers both."""
    acc, gyr = tilted_samples(1600, -0.7, 0.4, seed=3)
    got = dl.imu_static_initialization(acc, gyr, G)
    mean = acc.sum(axis=0) / len(acc)
    up = np.array([0.0, 0.0, 1.0])
    axis = np.cross(mean, up)
    angle = np.arccos(np.dot(mean, up) / np.linalg.norm(mean))
    want = Rotation.from_rotvec(axis / np.linalg.norm(axis) * angle).as_matrix()
    assert 0.5 < angle < 1.0
    assert np.abs(got["R"] - want).max() <= 64 * EPS
    # what the reference means by it: R turns the mean onto +z, and the bias is what the mean has beyond gravity
    turned = got["R"] @ mean
    assert np.abs(turned - np.array([0.0, 0.0, np.linalg.norm(mean)])).max() <= 64 * EPS * np.linalg.norm(mean)
    assert np.abs(got["ba"] - (mean - got["R"].T @ np.array([0.0, 0.0, G]))).max() <= 64 * EPS * G
    assert np.abs(got["bg"] - gyr.mean(axis=0)).max() <= 1600 * EPS * np.abs(gyr).max()
    assert abs(np.linalg.norm(got["ba"]) - abs(np.linalg.norm(mean) - G)) <= 64 * EPS * G


@pytest.mark.parametrize("mean,axis", [([0.0, 0.0, -G], [0.0, 1.0, 0.0]), ([1e-9, 0.0, -G], [-1.0, 0.0, 0.0]),
                                       ([0.0, -3e-9, -G], [0.0, 1.0, 0.0])])
def test_nearly_opposite_vectors_follow_the_written_rule(dl, mean, axis):
    """The accelerometer reads straight down: c < -1 + 1e-12.  The rule: half a turn about n(v0 x e_k), e_k the axis on
    which |v0| is least, ties the lowest k.  (0, 0, -1): k = 0, v0 x e_0 = (0, -1, 0) ... its sign does not matter to a
    half turn, the matrix is that of the stated axis."""
    got, want = dl.imu_static_initialization([mean], [[0.0, 0.0, 0.0]], G), il.static_initialization([mean], [[0.0, 0.0, 0.0]], G)
    assert want["opposite"] and same_bits(got["R"], want["R"]) and same_bits(got["ba"], want["ba"])
    half_turn = Rotation.from_rotvec(np.pi * np.array(axis)).as_matrix()
    assert np.abs(got["R"] - half_turn).max() <= 1e-8  # (the mean is 1e-9 off the axis)
    assert np.abs(got["R"] @ np.array(mean) - np.array([0.0, 0.0, G])).max() <= 1e-7


def test_just_outside_the_opposite_branch_is_eigens_general_one(dl):
    mean = [2e-6 * G, 0.0, -G]  # c = -1 + 2e-12
    got, want = dl.imu_static_initialization([mean], [[0.0, 0.0, 0.0]], G), il.static_initialization([mean], [[0.0, 0.0, 0.0]], G)
    assert not want["opposite"] and same_bits(got["R"], want["R"])


def test_refusals(dl):
    L = dl.load_library()
    one = np.array([0.1, 0.2, 9.7])
    out = [np.zeros(9), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)]
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def status(n, acc, gyr, g):
        return L.dliom_imu_static_initialization(n, None if acc is None else p(acc), p(gyr), C.c_double(g), *[p(o) for o in out])

    assert status(1, one, one, G) == dl.OK
    bad = one.copy()
    bad[1] = np.nan
    for args in ((0, one, one, G), (-1, one, one, G), (1, None, one, G), (1, bad, one, G), (1, one, bad, G), (1, np.zeros(3), one, G),
                 (1, one, one, 0.0), (1, one, one, -G), (1, one, one, float("inf")), (1, one, one, float("nan"))):
        assert status(*args) == dl.ERR_INVALID_ARGUMENT, args


def test_the_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """imu_lidar_init.cc and a stand-alone driver with its own main, built with -fsanitize=address,undefined and run as a
    program of its own: no library is loaded into it and nothing is preloaded"""
    exe = str(tmp_path / "imu_lidar_init_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "d-liom_amd", "csrc", "imu_lidar_init.cc"),
                           os.path.join(ROOT, "tests", "cpp", "imu_lidar_init_driver.cc")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and "runtime error" not in run.stderr


# ---- Initializer::Initialization and AlignWithWorld against the numpy model --------------------------------------------------
import imu_lidar_init_scenes as sc  # noqa: E402

_SCENES = {}


def scene(dl, **kwargs):
    """Frames, the truth and the model's result of a scene, computed once and left unchanged"""
    key = tuple(sorted(kwargs.items()))
    if key not in _SCENES:
        frames, truth = sc.frames_of(dl, **kwargs)
        _SCENES[key] = (frames, truth, il.align_with_world(frames, sc.TRANSFORM_LB, sc.G), il.initialization(frames, sc.TRANSFORM_LB, sc.G))
    return _SCENES[key]


def solver_bound(model):
    """The sum over the model's solves of 64 * cond(A) * 2^-52 * |x|: each solve may differ that much between the library's
    elimination and LAPACK's, and a later pass does not magnify what an earlier one left (it corrects g0 towards the same
    fixed point, at fixed norm), so the sum bounds the final unknowns.  cond(A) is computed by the model, not chosen."""
    assert model["solves"]
    return sum(s["bound"] for s in model["solves"])


def test_eight_frames_under_an_accelerating_turning_motion(dl):
    """8 frames, 0.1 s apart, noise-free 200 Hz IMU through dliom_imu_integrator, exact relative poses.  The reference's own
    acceptance holds (success, | |g| - g_norm | < 0.2); the library lies within the derived bound of the model; the model's
    values stay clear of every gate by more than that bound.  Measured with the model on a CPU: the gravity direction is
    0.0015 degrees and the last frame's velocity 1.3e-4 m/s (of 3.2) from the truth -- the mid-point rule's error at 200 Hz."""
    frames, truth, want, want_init = scene(dl)
    bound = solver_bound(want)
    got = dl.imu_lidar_align_with_world(frames, sc.TRANSFORM_LB, sc.G)
    got_init = dl.imu_lidar_initialization(frames, sc.TRANSFORM_LB, sc.G)
    print("bound", bound, "conds", [s["cond"] for s in want["solves"]], "excitation", want["excitation"], "gap", want["approximate_norm_gap"])
    # the gates: 0.25, 1.0, 0.2
    assert want["excitation"] - 0.25 > bound and want["approximate_norm_gap"] < 1.0 - bound
    assert abs(np.linalg.norm(want["gravity_in_laser"]) - sc.G) < 0.2 - bound
    assert got["outcome"] == want["outcome"] == il.OK and got_init["outcome"] == want_init["outcome"] == il.OK
    assert abs(np.linalg.norm(got["gravity_in_laser"]) - sc.G) < 0.2  # the reference's acceptance
    assert abs(got["excitation"] - want["excitation"]) <= 64 * EPS * want["excitation"]
    # the unknowns of the solves
    assert np.abs(got_init["velocities"] - want_init["velocities"]).max() <= bound
    assert np.abs(got_init["gravity"] - want_init["gravity"]).max() <= bound
    assert np.abs(got["gravity_in_laser"] - want["gravity_in_laser"]).max() <= bound
    # what is made of them: a rotation's entries move by |dg| / |g|, a vector turned by it by that times its length
    scale = max(1.0, np.abs(want["P"]).max(), np.abs(want["V"]).max())
    assert np.abs(got["world_rotation"] - want["world_rotation"]).max() <= bound
    assert np.abs(got["R"] - want["R"]).max() <= bound
    assert np.abs(got["P"] - want["P"]).max() <= bound * scale and np.abs(got["V"] - want["V"]).max() <= bound * scale
    # the measurement, from the model
    g, t = want["gravity_in_laser"], truth["gravity_in_laser"]
    angle = np.degrees(np.arccos(min(1.0, g @ t / np.linalg.norm(g) / np.linalg.norm(t))))
    velocity_error = np.linalg.norm(want["local_velocities"][-1] - truth["local_velocities"][-1])
    print("gravity direction error (degrees)", angle, "last velocity error (m/s)", velocity_error)
    assert angle < 0.01 and velocity_error < 1e-3
    # the world frame: gravity points down, and frame 0 keeps its position up to the lever arm
    down = got["world_rotation"] @ (-got["gravity_in_laser"])
    assert np.abs(down / np.linalg.norm(down) - np.array([0.0, 0.0, -1.0])).max() <= 64 * EPS
    for R in got["R"]:
        assert np.abs(R @ R.T - np.eye(3)).max() <= 64 * EPS


def test_frame_0_without_a_preintegration(dl):
    """Frame 0's own preintegration is never read: with and without it the bytes are the same"""
    frames, _, want, _ = scene(dl)
    bare, _, want_bare, _ = scene(dl, frame0_preintegration=False)
    assert bare[0][1] is None and want_bare["outcome"] == il.OK
    a, b = dl.imu_lidar_align_with_world(frames, sc.TRANSFORM_LB, sc.G), dl.imu_lidar_align_with_world(bare, sc.TRANSFORM_LB, sc.G)
    assert b["outcome"] == il.OK
    for key in ("P", "R", "V", "gravity_in_laser", "world_rotation"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert np.abs(b["V"] - want_bare["V"]).max() <= solver_bound(want_bare) * max(1.0, np.abs(want_bare["V"]).max())


def test_a_platform_at_rest_fails_the_excitation_gate(dl):
    frames, _, want, want_init = scene(dl, at_rest=True)
    got = dl.imu_lidar_align_with_world(frames, sc.TRANSFORM_LB, sc.G)
    assert want["excitation"] < 0.25 - 1e-6 and got["excitation"] < 0.25 - 1e-6
    assert got["outcome"] == want["outcome"] == il.NO_EXCITATION and not got["P"].any() and not got["V"].any()


def test_six_frames_fail_approximate_gravity(dl):
    frames, _, want, want_init = scene(dl, num_frames=6)
    assert want["excitation"] > 0.25 + 1e-6  # the gate before it is passed
    got, got_init = dl.imu_lidar_align_with_world(frames, sc.TRANSFORM_LB, sc.G), dl.imu_lidar_initialization(frames, sc.TRANSFORM_LB, sc.G)
    assert got["outcome"] == want["outcome"] == il.TOO_FEW_FRAMES and got_init["outcome"] == want_init["outcome"] == il.TOO_FEW_FRAMES
    seven, _, want7, _ = scene(dl, num_frames=7)
    assert dl.imu_lidar_align_with_world(seven, sc.TRANSFORM_LB, sc.G)["outcome"] == want7["outcome"] == il.OK


def test_an_approximate_gravity_off_by_more_than_one_fails_its_gate(dl):
    """The preintegrations of the scene with delta_v scaled by 1.3: the model's first solve misses g_norm by far more than
    1.0, and both stop there"""
    frames, _, _, _ = scene(dl)
    bent = [(pose, None if pre is None else dict(pre, delta_v=1.3 * pre["delta_v"], delta_p=1.3 * pre["delta_p"])) for pose, pre in frames]
    want = il.initialization(bent, sc.TRANSFORM_LB, sc.G)
    assert want["outcome"] == il.GRAVITY_NORM and want["approximate_norm_gap"] > 1.0 + solver_bound(want) and len(want["solves"]) == 1
    assert dl.imu_lidar_initialization(bent, sc.TRANSFORM_LB, sc.G)["outcome"] == il.GRAVITY_NORM


def test_refusals_of_the_two_calls(dl):
    L = dl.load_library()
    frames, _, _, _ = scene(dl)
    raw = dl._init_frames(frames)
    lb = sc.TRANSFORM_LB.copy()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    V, g, P, R, Rw, e, outcome = np.zeros(24), np.zeros(3), np.zeros(24), np.zeros(72), np.zeros(9), np.zeros(1), C.c_int()

    def init(fr, n, tlb, gn):
        return L.dliom_imu_lidar_initialization(fr, n, None if tlb is None else p(tlb), C.c_double(gn), p(V), p(g), C.byref(outcome))

    def align(fr, n, tlb, gn):
        return L.dliom_imu_lidar_align_with_world(fr, n, None if tlb is None else p(tlb), C.c_double(gn), p(P), p(R), p(V), p(g), p(Rw), p(e),
                                                  C.byref(outcome))

    assert init(raw, 8, lb, sc.G) == dl.OK and align(raw, 8, lb, sc.G) == dl.OK
    bad_lb = lb.copy()
    bad_lb[1] = np.inf
    for call in (init, align):
        for args in ((None, 8, lb, sc.G), (raw, 0, lb, sc.G), (raw, dl.INIT_MAX_FRAMES + 1, lb, sc.G), (raw, 8, None, sc.G),
                     (raw, 8, bad_lb, sc.G), (raw, 8, lb, 0.0), (raw, 8, lb, float("nan"))):
            assert call(*args) == dl.ERR_INVALID_ARGUMENT, (call.__name__, args[1:])
    assert align(raw, 1, lb, sc.G) == dl.ERR_INVALID_ARGUMENT
    for field, value in (("sum_dt", 0.0), ("sum_dt", float("nan"))):
        broken = dl._init_frames(frames)
        setattr(broken[3], field, value)
        assert init(broken, 8, lb, sc.G) == dl.ERR_INVALID_ARGUMENT and align(broken, 8, lb, sc.G) == dl.ERR_INVALID_ARGUMENT
    broken = dl._init_frames(frames)
    broken[2].pose[4] = float("nan")
    assert init(broken, 8, lb, sc.G) == dl.ERR_INVALID_ARGUMENT
