"""Shared by tests/test_pose_graph_landmarks_host.py, tests/test_gpu_pose_graph_landmarks.py and tools/pose_graph_bench.py:
restates the reference's interpolation and GetInitialLandmarkPose, makes the graphs with landmark observations and holds
their fixed case list.  The graphs without landmarks are pose_graph_terms_common's, the CPU model's harness is
pose_graph_common's."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
import pose_graph_terms_common as tc  # noqa: E402
from pose_graph_common import synth  # noqa: E402

OBSERVATION = np.dtype({"names": ["landmark", "prev_node", "next_node", "interpolation_parameter", "landmark_to_tracking",
                                  "translation_weight", "rotation_weight"],
                        "formats": ["<i4", "<i4", "<i4", "<f8", ("<f8", 7), "<f8", "<f8"], "offsets": [0, 4, 8, 16, 24, 80, 88],
                        "itemsize": 96})


class Graph(tc.Graph):
    """pose_graph_terms_common.Graph and: landmarks (L, 7), landmark_constant (uint8 a landmark), observations
    (OBSERVATION)."""

    def __init__(self, base, landmarks=None, landmark_constant=None, observations=None, **options):
        if not isinstance(base, tc.Graph):
            base = tc.Graph(base)
        tc.Graph.__init__(self, base, base.frames, base.frame_constraints, base.huber_scale, base.inter_submap, **options)
        self.landmarks = np.ascontiguousarray(np.zeros((0, 7)) if landmarks is None else landmarks, dtype=np.float64).reshape(-1, 7)
        self.landmark_constant = (np.zeros(len(self.landmarks), np.uint8) if landmark_constant is None
                                  else np.asarray(landmark_constant, np.uint8))
        self.observations = np.ascontiguousarray(np.zeros(0, OBSERVATION) if observations is None else observations, dtype=OBSERVATION)

    def device(self, dl, ctx, entry=None):
        return dl.PoseGraph(ctx, self.submaps, self.nodes, self.constraints, self.submap_constant, self.node_constant,
                            self.gravity, self.fix_z, self.nonmonotonic, self.max_iterations, fixed_frame_poses=self.frames,
                            fixed_frame_constraints=self.frame_constraints, huber_scale=self.huber_scale,
                            inter_submap=self.inter_submap if self.inter_submap.any() else None, entry=entry,
                            landmarks=self.landmarks, landmark_constant=self.landmark_constant if self.landmark_constant.any() else None,
                            landmark_observations=self.observations)


# ---- the reference's host arithmetic, restated -------------------------------------------------------------------------------
def slerp_scales(prev_q, next_q, t):
    """SlerpQuaternions (cost_helpers_impl.h:103-131) -> (prev_scale, next_scale, cos_theta)."""
    cos_theta = prev_q[0] * next_q[0] + prev_q[1] * next_q[1] + prev_q[2] * next_q[2] + prev_q[3] * next_q[3]
    prev_scale, next_scale = 1.0 - t, t
    if abs(cos_theta) < 1.0 - 1e-5:
        theta = np.arccos(abs(cos_theta))
        prev_scale, next_scale = np.sin((1.0 - t) * theta) / np.sin(theta), np.sin(t * theta) / np.sin(theta)
    if cos_theta < 0.0:
        next_scale = -next_scale
    return prev_scale, next_scale, cos_theta


def interpolate(prev_pose, next_pose, t):
    """InterpolateNodes3D (:133-153): the rotation is not renormalised."""
    a, b, _ = slerp_scales(prev_pose[3:], next_pose[3:], t)
    return np.concatenate([prev_pose[:3] + t * (next_pose[:3] - prev_pose[:3]), a * prev_pose[3:] + b * next_pose[3:]])


def _eigen_rotate(q, v):
    """Eigen's quaternion * vector, which is not q v q^-1 for a quaternion off the unit sphere."""
    uv = 2.0 * np.cross(q[1:], v)
    return v + q[0] * uv + np.cross(q[1:], uv)


def initial_landmark_pose(prev_pose, next_pose, t, landmark_to_tracking):
    """GetInitialLandmarkPose (optimization_problem_3d.cc:106-122): FromArrays(interpolated) * landmark_to_tracking."""
    pose = interpolate(prev_pose, next_pose, t)
    q = synth._quat_mul(pose[3:], landmark_to_tracking[3:])
    return np.concatenate([_eigen_rotate(pose[3:], landmark_to_tracking[:3]) + pose[:3], q / np.linalg.norm(q)])


def landmark_residual(observation, prev_pose, next_pose, landmark_pose):
    """LandmarkCostFunction3D in numpy, written from the formulas (not from the model's code): for the independent checks."""
    pose = interpolate(prev_pose, next_pose, observation["interpolation_parameter"])
    z = observation["landmark_to_tracking"]
    conj = np.array([1.0, -1.0, -1.0, -1.0])
    h_translation = _eigen_rotate(pose[3:] * conj, landmark_pose[:3] - pose[:3])
    q = synth._quat_mul(synth._quat_mul(landmark_pose[3:] * conj, pose[3:]), z[3:])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    angle = 2.0 * np.arctan2(np.linalg.norm(q[1:]), q[0])
    scale = 2.0 if angle < 1e-7 else angle / np.sin(angle / 2.0)
    return np.concatenate([(z[:3] - h_translation) * observation["translation_weight"], scale * q[1:] * observation["rotation_weight"]])


# ---- graphs with landmarks ---------------------------------------------------------------------------------------------------
def _noise(rng, noise):
    return np.concatenate([rng.normal(0, noise[0], 3), synth._quat_of(rng.normal(0, noise[1], 3))])


def observe(nodes, landmark_pose, landmark, prev_node, next_node, t, rng, noise=(0.02, 0.005), weights=(1e3, 1e1)):
    """One OBSERVATION row: the landmark at `landmark_pose` seen from the pose interpolated between nodes[prev_node] and
    nodes[next_node], with noise."""
    pose = interpolate(nodes[prev_node], nodes[next_node], t)
    pose[3:] /= np.linalg.norm(pose[3:])
    z = synth.pose7_compose(synth.pose7_compose(synth.pose7_inverse(pose), landmark_pose), _noise(rng, noise))
    return (landmark, prev_node, next_node, t, z, weights[0], weights[1])


def rows_to_observations(rows):
    out = np.zeros(len(rows), dtype=OBSERVATION)
    for i, row in enumerate(rows):
        out[i] = row
    return out


def with_landmarks(base, truth_nodes, landmark_truth, sightings, seed=0, start="initial", landmark_constant=None, **kw):
    """Adds landmarks to a graph whose nodes' true poses are known.  landmark_truth: (L, 7); sightings: a list of (landmark,
    prev_node, t) -- next_node is prev_node + 1.  start: "initial" for GetInitialLandmarkPose of the landmark's first
    observation at the graph's node poses, "truth" for the true poses (a landmark with a global_landmark_pose)."""
    rng = np.random.RandomState(3000 + seed)
    rows = [observe(truth_nodes, landmark_truth[l], l, p, p + 1, t, rng, **kw) for l, p, t in sightings]
    observations = rows_to_observations(rows)
    poses = np.array(landmark_truth, dtype=np.float64).reshape(-1, 7).copy()
    if start == "initial":
        for l in range(len(poses)):
            first = observations[np.flatnonzero(observations["landmark"] == l)[0]]
            poses[l] = initial_landmark_pose(base.nodes[first["prev_node"]], base.nodes[first["next_node"]],
                                             first["interpolation_parameter"], first["landmark_to_tracking"])
    return Graph(base, poses, landmark_constant, observations)


def some_landmarks(count, seed):
    rng = np.random.RandomState(4000 + seed)
    return np.array([np.concatenate([rng.uniform(-5, 5, 3), synth._quat_of(rng.uniform(-1.5, 1.5, 3))]) for _ in range(count)])


def evaluate_graph(fix_z):
    """The evaluation's case: 4 submaps, 40 nodes (0..13 frozen with the first submap), 3 landmarks (the last constant), 14
    observations that hold every branch; see EVALUATE_ROWS."""
    base, _, _ = tc.synthetic(4, 40, 0, seed=51, frozen_submaps=1, fix_z=fix_z)
    assert list(np.flatnonzero(base.node_constant)) == list(range(14))
    nodes = base.nodes.copy()
    nodes[17, 3:] = nodes[16, 3:]                                                    # identical rotations: the linear branch
    nodes[19, 3:] = synth._quat_mul(nodes[18, 3:], synth._quat_of([0.3, -1.9, 0.8]))  # a large relative rotation
    nodes[21, 3:] = -nodes[21, 3:]                                                   # cos theta < 0
    base = pc.Graph(base.submaps, nodes, base.constraints, base.submap_constant, base.node_constant, base.gravity, base.fix_z,
                    base.nonmonotonic, base.max_iterations)
    landmarks = some_landmarks(3, 51)
    rng = np.random.RandomState(51)
    rows = [observe(nodes, landmarks[l], l, p, n, t, rng, noise=(0.1, 0.1), weights=(3.0 + l, 7.0 + i))
            for i, (l, p, n, t) in enumerate(EVALUATE_ROWS)]
    return Graph(base, landmarks, [0, 0, 1], rows_to_observations(rows))


# (landmark, prev, next, t)
EVALUATE_ROWS = [
    (0, 16, 17, 0.3),   # the linear branch
    (0, 18, 19, 0.6),   # the slerp branch, a large relative rotation
    (0, 20, 21, 0.5),   # next.q negated
    (0, 25, 26, 0.0),   # t = 0
    (0, 25, 26, 1.0),   # t = 1
    (1, 26, 27, 0.25),  # node 26: promoted by two landmarks, constrained to two submaps
    (1, 30, 31, 0.7),
    (1, 13, 14, 0.5),   # prev on the frozen trajectory, next promoted
    (1, 2, 3, 0.2),     # both nodes constant, the landmark free
    (2, 33, 34, 0.5),   # the constant landmark seen from free nodes
    (2, 3, 4, 0.4),     # all six blocks constant: the fixed cost only
    (2, 36, 35, 0.8),   # prev behind next in the nodes' order
    (0, 38, 39, 0.9),
    (1, 38, 39, 0.1),
]


def boundary_graph(num_promoted_pairs, num_landmarks, fix_z=True, num_submaps=3, seed=61):
    """A step case whose reduced dimension is reached through promoted nodes and landmarks: the node pairs (2 k, 2 k + 1),
    k < num_promoted_pairs, each see one landmark.  Under fix_z with 3 submaps: 2 + 5 + 5 columns of the submaps, 5 a
    promoted node, 6 a landmark."""
    base, truth, _ = tc.synthetic(num_submaps, max(60, 2 * num_promoted_pairs + 4), 1, seed=seed, fix_z=fix_z)
    sightings = [(k % num_landmarks, 2 * k, 0.2 + 0.6 * (k % 7) / 7.0) for k in range(num_promoted_pairs)]
    return with_landmarks(base, truth, some_landmarks(num_landmarks, seed), sightings, seed=seed)


STEP_CASES = {
    # name -> (promoted pairs, landmarks, fix_z, reduced dimension)
    "dimension_256": (22, 4, True, 256),   # 12 + 44 * 5 + 4 * 6: the last size of the one-workgroup factorisation
    "dimension_260": (20, 8, True, 260),   # 12 + 40 * 5 + 8 * 6: the first size of the chip-wide one
    "dimension_86": (5, 2, False, 86),     # 14 + 10 * 6 + 2 * 6: the panel boundaries 32 and 64 inside the promoted nodes
}


def _every(n, stride, landmarks, offset=0):
    """Every `stride`-th node pair sees a landmark, the landmarks in turn."""
    return [((i // stride) % landmarks, i, 0.15 + 0.7 * ((i // stride) % 5) / 5.0) for i in range(offset, n - 1, stride)]


def _initial(e, d):
    base, truth, _ = tc.synthetic(3, 30, 0, seed=71, max_iterations=30)
    return with_landmarks(base, truth, some_landmarks(3, 71), _every(30, 4, 3), seed=71)


def _frames_and_loss(e, d):
    base, truth, inter = tc.synthetic(6, 120, 1, seed=42, max_iterations=50)
    g, inter = tc.false_closure(base, inter, truth, 5.0, submap=1, node=70, seed=42)
    g = tc.with_fixed_frames(g, truth, [dict(origin=tc._yaw_pose([1.0, 2.0, 0.0], -0.4), nodes=list(range(0, 120, 5)))], seed=42,
                             huber_scale=tc.LOSS_HUBER_SCALE, inter_submap=inter)
    return with_landmarks(g, truth, some_landmarks(4, 72), _every(120, 10, 4), seed=72)


def _frozen(e, d):
    # frozen_trajectories non-empty: every landmark constant, each with a global_landmark_pose (its start value)
    base, truth, _ = tc.synthetic(4, 40, 0, seed=73, frozen_submaps=2, max_iterations=30)
    return with_landmarks(base, truth, some_landmarks(3, 73), _every(40, 4, 3), seed=73, start="truth", landmark_constant=[1, 1, 1])


def _rejects(e, d):
    # (the 12 x 240 graph of pose_graph_terms_common's rejecting case passes the honesty test as well, but the model's
    # structured QR takes 19 s on it)
    base, truth, _ = tc.synthetic(6, 120, 1, seed=4, drift=(1.0, 0.6), max_iterations=30)
    return with_landmarks(base, truth, some_landmarks(8, 74), _every(120, 10, 8), seed=74)


def loop_pair():
    """One landmark seen at both ends of a drifting trajectory without loop closures -> (Graph with it, Graph without,
    truth)."""
    base, truth, _ = tc.synthetic(6, 120, 0, seed=75, drift=(0.1, 0.01), max_iterations=50)
    with_it = with_landmarks(base, truth, some_landmarks(1, 75), [(0, 0, 0.5), (0, 118, 0.5)], seed=75, noise=(0.005, 0.001),
                             weights=(1e4, 1e2))
    return with_it, Graph(base), truth


def _loop(e, d):
    return loop_pair()[0]


# The fixed list of full solves with landmarks: name -> a function of the model's executable and a directory.  Every case
# passes the honesty conditions of tests/test_pose_graph_landmarks_host.py (a case that does not is replaced here, never
# skipped there).
CASES = {
    "s3_n30_initial_landmark_pose": _initial,
    "s6_n120_landmarks_frames_loss": _frames_and_loss,
    "s4_n40_frozen_landmarks": _frozen,
    "s6_n120_landmarks_rejects_30": _rejects,
    "s6_n120_one_landmark_closes_the_loop": _loop,
}
REJECTING = ("s6_n120_landmarks_rejects_30",)


# ---- the adapter: optimization_problem_3d.cc:124-186 restated on the layout of tests/cpp/pose_graph_landmarks_adapter.cc ----
def adapter_node_order(num_nodes, extra):
    """The file's node j is NodeId{j % 2, j // 2}; MapById order is trajectory 0 (even j), trajectory 1 (odd j), then the
    extra node of trajectory 2 (index num_nodes)."""
    return list(range(0, num_nodes, 2)) + list(range(1, num_nodes, 2)) + ([num_nodes] if extra else [])


def adapter_compact(initial_pose, node_poses, spec, frozen, extra):
    """AddLandmarkCostFunctions' host steps -> (landmark indices in use, start poses (L, 7), constant flags, OBSERVATION rows on
    compact node indices).  node_poses: (N, 7) in the file's order; spec: a landmark a dict(pose = the global_landmark_pose or
    None, observations = [(trajectory, time, landmark_to_tracking, translation_weight, rotation_weight)]); frozen: the frozen
    trajectory or -1; initial_pose: GetInitialLandmarkPose (the binding's)."""
    n = len(node_poses)
    order = adapter_node_order(n, extra)
    compact = {j: i for i, j in enumerate(order)}
    poses = {j: (node_poses[j] if j < n else np.array([0.0, 0, 0, 1, 0, 0, 0])) for j in order}
    trajectories = {0: [(1000 + j * 10000000, j) for j in range(0, n, 2)], 1: [(1000 + j * 10000000, j) for j in range(1, n, 2)]}
    if extra:
        trajectories[2] = [(1000, n)]
    freeze = frozen >= 0
    used, starts, rows = [], [], []
    for l, landmark in enumerate(spec):
        if landmark["pose"] is None and freeze:
            continue
        added = False
        for trajectory, time, z, translation_weight, rotation_weight in landmark["observations"]:
            nodes = trajectories.get(trajectory, [])
            if not nodes or time < nodes[0][0]:
                continue
            at = next((i for i, (t, _) in enumerate(nodes) if t >= time), None)
            if at is None:
                continue
            if at == 0:
                at = 1
            if at == len(nodes):
                continue
            (prev_time, prev), (next_time, nxt) = nodes[at - 1], nodes[at]
            t = (float(time - prev_time) / 1e7) / (float(next_time - prev_time) / 1e7)
            if not added:
                starts.append(np.array(landmark["pose"]) if landmark["pose"] is not None else initial_pose(poses[prev], poses[nxt], t, z))
                used.append(l)
                added = True
            rows.append((len(used) - 1, compact[prev], compact[nxt], t, z, translation_weight, rotation_weight))
    return used, np.array(starts).reshape(-1, 7), np.full(len(used), 1 if freeze else 0, np.uint8), rows_to_observations(rows)


def adapter_case():
    """-> (pose_graph_common.Graph, truth, landmark spec) for adapter_compact: every skip rule, the first node's exact time,
    a landmark with and without a global pose, one none of whose observations is used."""
    base, truth, _ = tc.synthetic(5, 31, 0, seed=91, max_iterations=12)
    rng = np.random.RandomState(91)
    places = some_landmarks(4, 91)
    node_time = lambda j: 1000 + j * 10000000  # noqa: E731

    def seen(l, trajectory, time):
        """the landmark from the trajectory's true pose at `time` (between the nodes of that trajectory around it)"""
        js = [j for j in range(trajectory, len(truth), 2)]
        after = next((j for j in js if node_time(j) >= time), js[-1])
        after = max(after, js[1])
        before = after - 2
        t = (time - node_time(before)) / float(node_time(after) - node_time(before))
        pose = interpolate(truth[before], truth[after], min(max(t, 0.0), 1.0))
        pose[3:] /= np.linalg.norm(pose[3:])
        z = synth.pose7_compose(synth.pose7_compose(synth.pose7_inverse(pose), places[l]), _noise(rng, (0.02, 0.005)))
        return (trajectory, time, z, 1e3 + l, 1e1 + l)
    identity = np.array([0.0, 0, 0, 1, 0, 0, 0])
    spec = [
        dict(pose=None, observations=[seen(0, 0, 500),                                  # before the trajectory's first node
                                      seen(0, 0, 1000),                                 # at it: next == begin takes the node after
                                      seen(0, 1, node_time(6)),                         # between nodes 5 and 7 of trajectory 1
                                      seen(0, 0, node_time(31)),                        # behind the last node: no next
                                      (2, 1000, identity, 1.0, 1.0), (2, 2000, identity, 1.0, 1.0),  # one node: no pair
                                      (3, 1000, identity, 1.0, 1.0),                    # a trajectory without nodes
                                      seen(0, 0, node_time(20) + 2500000)]),
        dict(pose=synth.pose7_compose(places[1], _noise(rng, (0.3, 0.05))),
             observations=[seen(1, 1, node_time(1) + 3000000), seen(1, 0, node_time(10) + 14000000), seen(1, 1, node_time(27))]),
        dict(pose=None, observations=[seen(2, 0, 999), seen(2, 1, node_time(1) - 1)]),  # nothing is used: no block
        dict(pose=None, observations=[seen(3, 1, node_time(13) + 10000000), seen(3, 0, node_time(24) + 1)]),
    ]
    return base, truth, spec


def adapter_write(path, base, spec, frozen, extra):
    pc.write_adapter_graph(base, path)
    with open(path, "ab") as f:
        f.write(struct.pack("<3i", frozen, int(extra), len(spec)))
        for landmark in spec:
            pose = landmark["pose"]
            f.write(struct.pack("<i7di", pose is not None, *(np.zeros(7) if pose is None else pose), len(landmark["observations"])))
            for trajectory, time, z, translation_weight, rotation_weight in landmark["observations"]:
                f.write(struct.pack("<iq9d", trajectory, time, *z, translation_weight, rotation_weight))
