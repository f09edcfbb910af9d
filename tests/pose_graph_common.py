"""Shared by tests/test_pose_graph*_host.py, tests/test_gpu_pose_graph*.py and tools/pose_graph_bench.py: builds and runs
the CPU model (tests/cpp/pose_graph_model.cc) on any of the graph classes, makes the graphs without further terms and holds
their fixed case list.  The graphs with fixed frames and the loss are pose_graph_terms_common's, those with landmarks
pose_graph_landmarks_common's."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
from dliom import synth  # noqa: E402

MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "pose_graph_model.cc")
CONSTRAINT = np.dtype([("submap", "<i4"), ("node", "<i4"), ("zbar", "<f8", 7), ("translation_weight", "<f8"),
                       ("rotation_weight", "<f8")])
QR, ELIMINATED, SPARSE_QR, LINEARISE_ONLY = 0, 1, 2, 3  # the model's linear solvers: dense QR of [J; D], eliminated normal equations, QR with
# the nodes' columns first and the structural zeros skipped


def build_model(directory):
    exe = os.path.join(str(directory), "pose_graph_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def build_structure_check(directory):
    """tests/cpp/pose_graph_structure_check.cc as a stand-alone program under sanitisers; it reads the model's input."""
    exe = os.path.join(str(directory), "pose_graph_structure_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pose_graph_structure_check.cc")])
    return exe


def structure_check_fields(line):
    """One "<path> ok columns 14 pairs 3 ..." line of the structure check -> dict(columns=14, pairs=3, ...)."""
    words = line.split()
    assert words[1] == "ok", line
    return {key: int(value) for key, value in zip(words[2::2], words[3::2])}


class Graph:
    """submaps (S, 7), nodes (N, 7), constraints (CONSTRAINT), constant flags, gravity-aligned submap, options."""

    def __init__(self, submaps, nodes, constraints, submap_constant=None, node_constant=None, gravity=0, fix_z=False,
                 nonmonotonic=False, max_iterations=10):
        self.submaps = np.ascontiguousarray(submaps, dtype=np.float64).reshape(-1, 7)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 7)
        self.constraints = np.ascontiguousarray(constraints, dtype=CONSTRAINT)
        self.submap_constant = np.zeros(len(self.submaps), np.uint8) if submap_constant is None else np.asarray(submap_constant, np.uint8)
        self.node_constant = np.zeros(len(self.nodes), np.uint8) if node_constant is None else np.asarray(node_constant, np.uint8)
        self.gravity, self.fix_z, self.nonmonotonic, self.max_iterations = gravity, fix_z, nonmonotonic, max_iterations

    def with_options(self, **kw):
        g = Graph(self.submaps, self.nodes, self.constraints, self.submap_constant, self.node_constant, self.gravity, self.fix_z,
                  self.nonmonotonic, self.max_iterations)
        for k, v in kw.items():
            assert hasattr(g, k), k
            setattr(g, k, v)
        return g

    def device(self, dl, ctx):
        return dl.PoseGraph(ctx, self.submaps, self.nodes, self.constraints, self.submap_constant, self.node_constant,
                            self.gravity, self.fix_z, self.nonmonotonic, self.max_iterations)


def _terms(graph):
    """The further terms of any of the graph classes (this module's Graph, pose_graph_terms_common's, pose_graph_landmarks_
    common's), an absent one empty -> (frames, frame_constraints, huber_scale, inter_submap, landmarks, landmark_constant,
    observations)."""
    frames, landmarks = getattr(graph, "frames", np.zeros((0, 7))), getattr(graph, "landmarks", np.zeros((0, 7)))
    return (frames, getattr(graph, "frame_constraints", np.zeros(0, CONSTRAINT)), getattr(graph, "huber_scale", 0.0),
            getattr(graph, "inter_submap", np.zeros(len(graph.constraints), np.uint8)), landmarks,
            getattr(graph, "landmark_constant", np.zeros(len(landmarks), np.uint8)), getattr(graph, "observations", np.zeros(0, np.uint8)))


def _write(graph, path, mode, solver, radius):
    """The model's input (tests/cpp/pose_graph_model.cc, above its main)."""
    frames, frame_constraints, huber_scale, inter_submap, landmarks, landmark_constant, observations = _terms(graph)
    with open(path, "wb") as f:
        f.write(struct.pack("<13i", len(graph.submaps), len(graph.nodes), len(graph.constraints), graph.gravity, int(graph.fix_z),
                            int(graph.nonmonotonic), graph.max_iterations, mode, solver, len(frames), len(frame_constraints),
                            len(landmarks), len(observations)))
        f.write(struct.pack("<2d", radius, huber_scale))
        f.write(graph.submaps.tobytes() + frames.tobytes() + graph.nodes.tobytes())
        f.write(np.concatenate([graph.submap_constant, graph.node_constant]).astype("<i4").tobytes())
        f.write(graph.constraints.tobytes() + frame_constraints.tobytes())
        f.write(inter_submap.astype("<i4").tobytes())
        f.write(landmarks.tobytes() + landmark_constant.astype("<i4").tobytes() + observations.tobytes())


def write_adapter_graph(graph, path):
    """The head of the adapter programs' input (tests/cpp/pose_graph*_adapter.cc): the graph without further terms."""
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", len(graph.submaps), len(graph.nodes), len(graph.constraints), graph.gravity, int(graph.fix_z),
                            int(graph.nonmonotonic), graph.max_iterations, 0, 0))
        f.write(struct.pack("<d", 1e4))
        f.write(graph.submaps.tobytes() + graph.nodes.tobytes())
        f.write(np.concatenate([graph.submap_constant, graph.node_constant]).astype("<i4").tobytes())
        f.write(graph.constraints.tobytes())


def _run(exe, graph, directory, mode, solver, radius=1e4):
    src, dst = os.path.join(str(directory), "pg_in.bin"), os.path.join(str(directory), "pg_out.bin")
    _write(graph, src, mode, solver, radius)
    subprocess.check_call([exe, src, dst])
    return open(dst, "rb").read()


def _split(graph, rows):
    """rows in the model's order (submaps, fixed frames, nodes, landmarks) -> (submaps, nodes, frames, landmarks), the order
    in which the device reports them"""
    s, f, n = len(graph.submaps), len(_terms(graph)[0]), len(graph.nodes)
    return rows[:s].copy(), rows[s + f:s + f + n].copy(), rows[s:s + f].copy(), rows[s + f + n:].copy()


def model_solve(exe, graph, directory, solver=ELIMINATED):
    """-> dict(termination, iterations, successful, unsuccessful, columns, steps, rises, initial_cost, final_cost,
    quality_margin, tolerance_margin, seconds, submaps, nodes, frames, landmarks, loss_margin, clamp_margin, clamped_steps,
    slerp_margin).  Of an absent term the margins are 1e300, slerp_margin inf, and clamped_steps is 0."""
    data = _run(exe, graph, directory, 0, solver)
    termination, iterations, successful, unsuccessful, columns, num_steps, rises, clamped = struct.unpack_from("<8i", data, 0)
    initial, final, quality, tolerance, seconds = struct.unpack_from("<5d", data, 32)
    steps = list(struct.unpack_from("<%di" % num_steps, data, 72))
    at = 72 + 4 * num_steps
    poses = np.frombuffer(data, dtype=np.float64, count=(len(data) - at - 24) // 8, offset=at).reshape(-1, 7)
    submaps, nodes, frames, landmarks = _split(graph, poses)
    assert (len(submaps), len(nodes), len(landmarks)) == (len(graph.submaps), len(graph.nodes), len(_terms(graph)[4]))
    loss_margin, clamp_margin, slerp_margin = struct.unpack_from("<3d", data, len(data) - 24)
    if len(landmarks) + len(_terms(graph)[6]) == 0:
        assert slerp_margin == 1e300
        slerp_margin = np.inf
    return dict(termination=termination, iterations=iterations, successful=successful, unsuccessful=unsuccessful,
                columns=columns, steps=steps, rises=rises, initial_cost=initial, final_cost=final, quality_margin=quality,
                tolerance_margin=tolerance, seconds=seconds, submaps=submaps, nodes=nodes, frames=frames, landmarks=landmarks,
                loss_margin=loss_margin, clamp_margin=clamp_margin, clamped_steps=clamped, slerp_margin=slerp_margin)


def _counts(graph):
    """-> (constraints and fixed-frame constraints, observations, poses)"""
    frames, frame_constraints, _, _, landmarks, _, observations = _terms(graph)
    return (len(graph.constraints) + len(frame_constraints), len(observations),
            len(graph.submaps) + len(frames) + len(graph.nodes) + len(landmarks))


def model_evaluate(exe, graph, directory):
    """-> (cost, residuals (C + CF + O, 6), gradient (S + N + F + L, 6) -- submaps, nodes, fixed frames, landmarks, as the
    device reports it --, columns)"""
    data = _run(exe, graph, directory, 1, 0)
    failed, columns = struct.unpack_from("<2i", data, 0)
    assert failed == 0
    cost = struct.unpack_from("<d", data, 8)[0]
    c, o, p = _counts(graph)
    r = np.frombuffer(data, dtype=np.float64, count=6 * (c + o), offset=16).reshape(c + o, 6).copy()
    g = np.frombuffer(data, dtype=np.float64, count=6 * p, offset=16 + 48 * (c + o)).reshape(p, 6)
    assert len(data) == 16 + 48 * (c + o + p)
    return cost, r, np.concatenate(_split(graph, g)), columns


def model_step(exe, graph, directory, solver, radius=1e4):
    """-> dict(delta (S + N + F + L, 6) in the device's order, model_cost_change, columns, blocks: the remaining constraints'
    and fixed-frame constraints' (c, r (6), js (6, 6), jn (6, 6)) arrays on the unscaled tangent slots, scale like delta)"""
    data = _run(exe, graph, directory, 2, solver, radius)
    failed, columns = struct.unpack_from("<2i", data, 0)
    assert failed == 0
    change = struct.unpack_from("<d", data, 8)[0]
    c, _, p = _counts(graph)
    delta = np.frombuffer(data, dtype=np.float64, count=6 * p, offset=16).reshape(p, 6)
    at = 16 + 48 * p
    block = np.dtype([("c", "<i4"), ("r", "<f8", 6), ("js", "<f8", (6, 6)), ("jn", "<f8", (6, 6))])
    blocks = struct.unpack_from("<i", data, at)[0]
    # the constraints' blocks come first; an observation's (c past the constraints) has a third 6 x 6 block
    two = 0
    while two < blocks and struct.unpack_from("<i", data, at + 4 + two * block.itemsize)[0] < c:
        two += 1
    rec = np.frombuffer(data, dtype=block, count=two, offset=at + 4)
    scale = np.frombuffer(data, dtype=np.float64, count=6 * p, offset=at + 4 + rec.nbytes + (blocks - two) * (block.itemsize + 288)).reshape(p, 6)
    assert len(data) == at + 4 + rec.nbytes + (blocks - two) * (block.itemsize + 288) + 48 * p
    return dict(delta=np.concatenate(_split(graph, delta)), model_cost_change=change, columns=columns, blocks=rec,
                scale=np.concatenate(_split(graph, scale)))


def reduces_noise(exe, directory):
    """The problem of optimization_problem_3d_test.cc:106-191 -> (Graph, ground truth node poses (100, 7))."""
    path = os.path.join(str(directory), "reduces_noise.bin")
    subprocess.check_call([exe, "--reduces-noise", path])
    data = open(path, "rb").read()
    s, n, c, gravity, fix_z, nonmonotonic, iterations, _, _ = struct.unpack_from("<9i", data, 0)
    at = 44
    poses = np.frombuffer(data, dtype=np.float64, count=7 * (s + n), offset=at).reshape(-1, 7)
    at += 56 * (s + n) + 4 * (s + n)
    constraints = np.frombuffer(data, dtype=CONSTRAINT, count=c, offset=at)
    truth = np.frombuffer(data, dtype=np.float64, count=7 * n, offset=at + 80 * c).reshape(n, 7)
    return Graph(poses[:s], poses[s:], constraints, gravity=gravity, fix_z=bool(fix_z), nonmonotonic=bool(nonmonotonic),
                 max_iterations=iterations), truth.copy()


def noise_errors(truth, nodes):
    """optimization_problem_3d_test.cc:158-187: sum of |dt| and of GetAngle(truth^-1 * node) over the nodes."""
    dt = np.linalg.norm(truth[:, :3] - nodes[:, :3], axis=1).sum()
    angle = 0.0
    for a, b in zip(truth, nodes):
        q = synth.pose7_compose(synth.pose7_inverse(a), b)[3:]
        angle += 2 * np.arctan2(np.linalg.norm(q[1:]), abs(q[0]))
    return dt, angle


def rotation_angles(a, b):
    """Per pose the angle of the relative rotation between the quaternions (w x y z) of a and b, whatever their sign and
    norm: 2 atan2(|vec|, |w|) of conj(a) * b."""
    qa, qb = a[:, 3:] / np.linalg.norm(a[:, 3:], axis=1)[:, None], b[:, 3:] / np.linalg.norm(b[:, 3:], axis=1)[:, None]
    w = np.abs((qa * qb).sum(axis=1))
    vec = np.stack([qa[:, 0] * qb[:, 1] - qa[:, 1] * qb[:, 0] - qa[:, 2] * qb[:, 3] + qa[:, 3] * qb[:, 2],
                    qa[:, 0] * qb[:, 2] + qa[:, 1] * qb[:, 3] - qa[:, 2] * qb[:, 0] - qa[:, 3] * qb[:, 1],
                    qa[:, 0] * qb[:, 3] - qa[:, 1] * qb[:, 2] + qa[:, 2] * qb[:, 1] - qa[:, 3] * qb[:, 0]], axis=1)
    return 2 * np.arctan2(np.linalg.norm(vec, axis=1), w)


def synthetic(num_submaps, num_nodes, loop_groups=0, seed=0, frozen_submaps=0, drift=(0.02, 0.002), **options):
    d = synth.pose_graph(num_submaps, num_nodes, loop_groups, seed, frozen_submaps=frozen_submaps, drift=drift)
    return Graph(d["submaps"], d["nodes"], d["constraints"], d["submap_constant"], d["node_constant"], **options)


def branches_graph(fix_z):
    """One small graph that holds every branch of the evaluation: a zero rotation residual (zbar = the current relative
    pose), a relative rotation near pi (w < 0 flip), the gravity-aligned first submap, a constant submap with a constant
    node (a fixed constraint), a node with 1 constraint, a node with 9, an unconstrained node, an unconstrained submap."""
    rng = np.random.RandomState(5)
    num_submaps, num_nodes = 11, 8

    def pose():
        return np.concatenate([rng.uniform(-3, 3, 3), synth._quat_of(rng.uniform(-1.5, 1.5, 3))])
    submaps = np.array([pose() for _ in range(num_submaps)])
    nodes = np.array([pose() for _ in range(num_nodes)])
    rows = []

    def relative(a, j):
        return synth.pose7_compose(synth.pose7_inverse(submaps[a]), nodes[j])

    def add(a, j, z, tw=3.0, rw=7.0):
        rows.append((a, j, z, tw, rw))
    noise = lambda: np.concatenate([rng.normal(0, 0.1, 3), synth._quat_of(rng.normal(0, 0.1, 3))])  # noqa: E731
    add(0, 0, relative(0, 0))                                  # zero residual, first submap
    add(1, 0, synth.pose7_compose(relative(1, 0), noise()))
    add(1, 1, synth.pose7_compose(relative(1, 1), np.concatenate([[0.1, 0, 0], synth._quat_of([0, 0, 3.1])])))  # near pi
    add(2, 1, synth.pose7_compose(relative(2, 1), np.concatenate([[0, 0.1, 0], -synth._quat_of([0.2, 0, 3.0])])))  # -q: w < 0
    add(0, 2, synth.pose7_compose(relative(0, 2), noise()))    # node 2: one constraint
    for a in range(9):                                         # node 3: nine constraints
        add(a, 3, synth.pose7_compose(relative(a, 3), noise()), 1.0 + a, 2.0 + a)
    add(9, 4, synth.pose7_compose(relative(9, 4), noise()))    # submap 9 and node 4 constant: a fixed constraint
    add(9, 5, synth.pose7_compose(relative(9, 5), noise()))    # constant submap, free node
    add(3, 4, synth.pose7_compose(relative(3, 4), noise()))    # free submap, constant node
    add(3, 3, synth.pose7_compose(relative(3, 3), noise()))    # a duplicate pair (3, 3)
    add(4, 6, synth.pose7_compose(relative(4, 6), noise()))
    add(5, 6, synth.pose7_compose(relative(5, 6), noise()))    # node 7 and submap 10: unconstrained
    constraints = np.zeros(len(rows), dtype=CONSTRAINT)
    for i, row in enumerate(rows):
        constraints[i] = row
    submap_constant, node_constant = np.zeros(num_submaps, np.uint8), np.zeros(num_nodes, np.uint8)
    submap_constant[9] = node_constant[4] = 1
    return Graph(submaps, nodes, constraints, submap_constant, node_constant, gravity=0, fix_z=fix_z)


# The fixed list of full solves: name -> a function of the model's executable and a directory.  Every case passes the
# honesty conditions of tests/test_pose_graph_host.py (a case that does not is replaced here, never skipped there).
def _noise(exe, directory):
    return reduces_noise(exe, directory)[0]


CASES = {
    "reduces_noise": _noise,
    "s12_n240_monotonic_10": lambda e, d: synthetic(12, 240, 2, seed=1, max_iterations=10),
    # a drift large enough that ten iterations do not converge: the iteration cap, NO_CONVERGENCE
    "s12_n240_drift_cap_10": lambda e, d: synthetic(12, 240, 2, seed=2, drift=(0.5, 0.1), max_iterations=10),
    # a rotational drift large enough that Levenberg-Marquardt rejects steps (the radius shrinks, the linearisation is kept),
    # and, non-monotonic, accepts steps after which the cost is higher (REJECTING / RISING below)
    "s12_n240_rejects_30": lambda e, d: synthetic(12, 240, 2, seed=2, drift=(0.5, 0.3), max_iterations=30),
    "s12_n240_rejects_b_30": lambda e, d: synthetic(12, 240, 2, seed=3, drift=(1.0, 0.6), max_iterations=30),
    "s12_n240_nonmonotonic_rises_16": lambda e, d: synthetic(12, 240, 2, seed=3, drift=(1.0, 0.6), nonmonotonic=True, max_iterations=16),
    "s12_n240_nonmonotonic_rises_b_16": lambda e, d: synthetic(12, 240, 2, seed=2, drift=(0.5, 0.3), nonmonotonic=True, max_iterations=16),
    "s12_n240_nonmonotonic_50": lambda e, d: synthetic(12, 240, 2, seed=2, nonmonotonic=True, max_iterations=50),
    "s12_n240_fix_z_50": lambda e, d: synthetic(12, 240, 1, seed=3, fix_z=True, max_iterations=50),
    "s12_n240_frozen_50": lambda e, d: synthetic(12, 240, 2, seed=4, frozen_submaps=3, max_iterations=50),
    "s44_n900_monotonic_10": lambda e, d: synthetic(44, 900, 4, seed=5, max_iterations=10),
    "s44_n900_nonmonotonic_50": lambda e, d: synthetic(44, 900, 4, seed=6, nonmonotonic=True, max_iterations=50),
}
# the cases small enough for the model's dense QR of [J; D] as LevenbergMarquardtStrategy has it (rows x columns^2
# operations a step); every case is solved with the structured QR (SPARSE_QR: the same factorisation, zeros skipped)
QR_CASES = ("reduces_noise",)
REJECTING = ("s12_n240_rejects_30", "s12_n240_rejects_b_30", "s12_n240_nonmonotonic_rises_16")  # cases with unsuccessful steps
RISING = ("s12_n240_nonmonotonic_rises_16", "s12_n240_nonmonotonic_rises_b_16")  # accepted steps that raise the cost
