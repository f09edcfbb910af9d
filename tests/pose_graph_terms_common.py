"""Shared by tests/test_pose_graph_terms_host.py, tests/test_gpu_pose_graph_terms.py and tools/pose_graph_bench.py: makes
the graphs with the further terms (fixed-frame pose constraints and the Huber loss) and holds their fixed case list.  The
graphs without a further term and the CPU model's harness are pose_graph_common's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_common as pc  # noqa: E402
from pose_graph_common import synth  # noqa: E402

CONSTRAINT = pc.CONSTRAINT


class Graph(pc.Graph):
    """pose_graph_common.Graph and: frames (F, 7), frame_constraints (CONSTRAINT, `submap` = the fixed frame),
    huber_scale, inter_submap (uint8 a constraint, or None = none)."""

    def __init__(self, base, frames=None, frame_constraints=None, huber_scale=0.0, inter_submap=None, **options):
        pc.Graph.__init__(self, base.submaps, base.nodes, base.constraints, base.submap_constant, base.node_constant,
                          base.gravity, base.fix_z, base.nonmonotonic, base.max_iterations)
        for k, v in options.items():
            assert hasattr(self, k), k
            setattr(self, k, v)
        self.frames = np.ascontiguousarray(np.zeros((0, 7)) if frames is None else frames, dtype=np.float64).reshape(-1, 7)
        self.frame_constraints = np.ascontiguousarray(np.zeros(0, CONSTRAINT) if frame_constraints is None else frame_constraints,
                                                      dtype=CONSTRAINT)
        self.huber_scale = float(huber_scale)
        self.inter_submap = np.zeros(len(self.constraints), np.uint8) if inter_submap is None else np.asarray(inter_submap, np.uint8)

    def device(self, dl, ctx, entry=None):
        return dl.PoseGraph(ctx, self.submaps, self.nodes, self.constraints, self.submap_constant, self.node_constant,
                            self.gravity, self.fix_z, self.nonmonotonic, self.max_iterations, fixed_frame_poses=self.frames,
                            fixed_frame_constraints=self.frame_constraints, huber_scale=self.huber_scale,
                            inter_submap=self.inter_submap if self.inter_submap.any() else None, entry=entry)


# ---- graphs with the further terms ------------------------------------------------------------------------------------------
def _yaw_pose(t, yaw):
    return np.concatenate([np.asarray(t, dtype=np.float64), synth._quat_of([0.0, 0.0, yaw])])


def with_fixed_frames(base, truth_nodes, frames, seed=0, noise=(0.05, 0.01), weights=(1e1, 1e2), **terms):
    """Adds fixed frames to a graph whose nodes' true poses are known.  frames: a list of dict(origin = the frame's true
    pose in the map (yaw only), nodes = the node indices that carry a fixed-frame pose, start = the block's start value or
    None for the fork's rule: the first constrained node's pose * zbar^-1, reduced to its yaw)."""
    rng = np.random.RandomState(1000 + seed)
    poses, rows = [], []
    for f, spec in enumerate(frames):
        first = None
        for j in spec["nodes"]:
            z = synth.pose7_compose(synth.pose7_inverse(spec["origin"]), truth_nodes[j])
            z = synth.pose7_compose(z, np.concatenate([rng.normal(0, noise[0], 3), synth._quat_of(rng.normal(0, noise[1], 3))]))
            rows.append((f, j, z, weights[0], weights[1]))
            if first is None:
                first = synth.pose7_compose(base.nodes[j], synth.pose7_inverse(z))
        start = spec.get("start")
        if start is None:
            start = yaw_only(first)
        poses.append(start)
    constraints = np.zeros(len(rows), dtype=CONSTRAINT)
    for i, row in enumerate(rows):
        constraints[i] = row
    return Graph(base, np.array(poses).reshape(-1, 7), constraints, **terms)


def get_yaw(q):
    """transform::GetYaw: the angle about z of the rotated x axis."""
    direction = synth._quat_rotate(q, np.array([1.0, 0.0, 0.0]))
    return np.arctan2(direction[1], direction[0])


def yaw_only(pose):
    """Rigid3d(translation, AngleAxis(GetYaw(rotation), UnitZ)) (optimization_problem_3d.cc:529-533)."""
    yaw = get_yaw(pose[3:])
    return np.concatenate([pose[:3], [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]])


def synthetic(num_submaps, num_nodes, loop_groups=0, seed=0, frozen_submaps=0, drift=(0.02, 0.002), **options):
    """pose_graph_common.synthetic and the nodes' true poses; the INTER_SUBMAP constraints are the loop closures (the rows
    behind the 2 N - ... INTRA_SUBMAP ones, weights 1e4 / 1e2)."""
    d = synth.pose_graph(num_submaps, num_nodes, loop_groups, seed, frozen_submaps=frozen_submaps, drift=drift)
    g = pc.Graph(d["submaps"], d["nodes"], d["constraints"], d["submap_constant"], d["node_constant"], **options)
    return g, d["truth_nodes"], (d["constraints"]["translation_weight"] == 1e4).astype(np.uint8)


def false_closure(base, inter_submap, truth_nodes, offset=5.0, submap=0, node=None, seed=0):
    """Appends one INTER_SUBMAP constraint whose zbar is `offset` metres wrong."""
    node = len(base.nodes) // 2 if node is None else node
    rng = np.random.RandomState(2000 + seed)
    # the submaps' true poses are their first nodes' (synth.pose_graph)
    segments = max(len(base.submaps) - 1, 1)
    start = min(submap * len(base.nodes) // segments, len(base.nodes) - 1)
    z = synth.pose7_compose(synth.pose7_inverse(truth_nodes[start]), truth_nodes[node])
    direction = rng.normal(0, 1, 3)
    z[:3] += offset * direction / np.linalg.norm(direction)
    row = np.zeros(1, dtype=CONSTRAINT)
    row[0] = (submap, node, z, 1e4, 1e2)
    g = pc.Graph(base.submaps, base.nodes, np.concatenate([base.constraints, row]), base.submap_constant, base.node_constant,
                 base.gravity, base.fix_z, base.nonmonotonic, base.max_iterations)
    return g, np.concatenate([inter_submap, [1]]).astype(np.uint8)


def node_error(truth_nodes, nodes):
    """Sum over the nodes of the distance to the truth."""
    return np.linalg.norm(truth_nodes[:, :3] - nodes[:, :3], axis=1).sum()


EVALUATE_HUBER_SCALE = 3e4  # among the norms of evaluate_graph's 34 tagged residual blocks (2.5e4 .. 3.9e4)


def evaluate_graph(fix_z, huber_scale):
    """The evaluation's case: 6 submaps x 200 nodes, the first submap and its nodes frozen, two groups of loop closures
    (tagged INTER_SUBMAP; with EVALUATE_HUBER_SCALE their s lies on both sides of huber_scale^2, which
    tests/test_pose_graph_terms_host.py asserts) and two fixed frames, the second on nodes of the frozen submap only."""
    base, truth, inter = synthetic(6, 200, 2, seed=21, frozen_submaps=1, drift=(0.05, 0.01), fix_z=fix_z)
    frozen = np.flatnonzero(base.node_constant)
    frames = [dict(origin=_yaw_pose([3.0, -2.0, 1.0], 0.4), nodes=list(range(60, 200, 7))),
              dict(origin=_yaw_pose([-1.0, 4.0, 0.5], -1.1), nodes=list(frozen[::5]))]
    return with_fixed_frames(base, truth, frames, seed=21, huber_scale=huber_scale, inter_submap=inter if huber_scale > 0 else None)


def boundary_graph(num_submaps, num_frames, fix_z):
    """A step case whose reduced dimension reaches the one-workgroup limit (padded 256) through fixed-frame columns."""
    base, truth, _ = synthetic(num_submaps, 2 * (num_submaps - 1), 1, seed=num_submaps, fix_z=fix_z)
    n = len(base.nodes)
    frames = [dict(origin=_yaw_pose([1.0 + f, -2.0, 0.3], 0.3 * (f + 1)), nodes=list(range(f, n, 3))) for f in range(num_frames)]
    return with_fixed_frames(base, truth, frames, seed=num_submaps)


def _one_frame(e, d):
    base, truth, _ = synthetic(3, 20, 0, seed=31, max_iterations=30)
    return with_fixed_frames(base, truth, [dict(origin=_yaw_pose([2.0, 1.0, 0.2], 0.5), nodes=list(range(20)))], seed=31)


def _clamped(e, d):
    base, truth, _ = synthetic(3, 20, 0, seed=32, max_iterations=40)
    origin = _yaw_pose([2.0, 1.0, 0.2], 0.5)
    return with_fixed_frames(base, truth, [dict(origin=origin, nodes=list(range(20)), start=_yaw_pose([2.0, 1.0, 0.2], 0.5 + 1.6))],
                             seed=32, weights=(1e1, 1e2))


def _frozen(e, d):
    base, truth, _ = synthetic(4, 40, 0, seed=33, frozen_submaps=2, max_iterations=30)
    frozen = list(np.flatnonzero(base.node_constant))
    free = list(np.flatnonzero(base.node_constant == 0))
    return with_fixed_frames(base, truth, [dict(origin=_yaw_pose([0.5, 0.0, 0.0], -0.7), nodes=frozen[::2]),
                                           dict(origin=_yaw_pose([-2.0, 1.0, 0.1], 0.2), nodes=free[::2])], seed=33)


def _mid_trajectory(e, d):
    base, truth, _ = synthetic(3, 20, 0, seed=34, max_iterations=30)
    return with_fixed_frames(base, truth, [dict(origin=_yaw_pose([1.0, -1.0, 0.0], 1.0), nodes=list(range(9, 20)))], seed=34)


def _nonmonotonic(e, d):
    base, truth, _ = synthetic(12, 240, 2, seed=3, drift=(1.0, 0.6), nonmonotonic=True, max_iterations=16)
    return with_fixed_frames(base, truth, [dict(origin=_yaw_pose([1.0, -1.0, 0.0], 1.0), nodes=list(range(0, 240, 4)))], seed=35)


def _rejects(e, d):
    # (seed 2 with the drift (0.5, 0.3) of pose_graph_common's rejecting case is not used: after its 30 iterations the model's
    # own two linear solvers are 3.5e-8 apart in the poses, above the 1e-8 of the honesty test)
    base, truth, _ = synthetic(12, 240, 2, seed=3, drift=(1.0, 0.6), max_iterations=30)
    return with_fixed_frames(base, truth, [dict(origin=_yaw_pose([1.0, -1.0, 0.0], 1.0), nodes=list(range(0, 240, 4)))], seed=36)


def loss_pair(huber_scale):
    """12 submaps x 20 nodes a submap on a known truth with one inter-submap constraint 5 m wrong -> (Graph, truth)."""
    base, truth, inter = synthetic(12, 240, 2, seed=41, max_iterations=50)
    g, inter = false_closure(base, inter, truth, 5.0, submap=1, node=150, seed=41)
    return Graph(g, huber_scale=huber_scale, inter_submap=inter if huber_scale > 0 else None), truth


# Between basic_config_3d.lua:108 (1e2) and campus.lua:20 (1e5).  With the loop closures' weight 1e4 and their 1 cm
# noise a true closure has s near 1e4 = (1e2)^2, on the loss's boundary, where no case can be honest (loss_margin); at 1e3
# the true closures lie inside the quadratic region (s about 3e4 << 1e6) and the 5 m closure far outside (2.5e9).
LOSS_HUBER_SCALE = 1e3


def _false_closure(e, d):
    return loss_pair(LOSS_HUBER_SCALE)[0]


def _loss_and_frames(e, d):
    base, truth, inter = synthetic(6, 120, 1, seed=42, max_iterations=50)
    g, inter = false_closure(base, inter, truth, 5.0, submap=1, node=70, seed=42)
    return with_fixed_frames(g, truth, [dict(origin=_yaw_pose([1.0, 2.0, 0.0], -0.4), nodes=list(range(0, 120, 5))),
                                        dict(origin=_yaw_pose([0.0, -3.0, 0.5], 2.0), nodes=list(range(60, 120, 3)))], seed=42,
                             huber_scale=LOSS_HUBER_SCALE, inter_submap=inter)


# The fixed list of full solves with further terms: name -> a function of the model's executable and a directory.  Every
# case passes the honesty conditions of tests/test_pose_graph_terms_host.py (a case that does not is replaced here, never
# skipped there).
CASES = {
    "s3_n20_one_frame": _one_frame,
    "s3_n20_clamped_yaw": _clamped,
    "s4_n40_frame_on_frozen": _frozen,
    "s3_n20_frame_from_mid_trajectory": _mid_trajectory,
    "s12_n240_frame_nonmonotonic_rises_16": _nonmonotonic,
    "s12_n240_frame_rejects_30": _rejects,
    "s12_n240_loss_false_closure": _false_closure,
    "s6_n120_loss_and_frames": _loss_and_frames,
}
CLAMPED = ("s3_n20_clamped_yaw",)  # cases with a yaw step clamped to 0.5
REJECTING = ("s12_n240_frame_rejects_30", "s12_n240_frame_nonmonotonic_rises_16")   # cases with unsuccessful steps
RISING = ("s12_n240_frame_nonmonotonic_rises_16",)  # accepted steps that raise the cost
LOSSY = ("s12_n240_loss_false_closure", "s6_n120_loss_and_frames")  # cases in which the loss leaves its quadratic region
