"""The CPU model of include/dliom.h "scan alignment by ICP", operation for operation: numpy float32 for the brute-force
nearest-neighbour search, numpy float64 element-wise sums for the fixed tree, Python floats for the solve and the
decisions.  The GPU tests compare bits against it; the host tests check it against scipy's kd-tree, math.fsum and
numpy's SVD."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "d-liom_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dliom import synth  # noqa: E402

JACOBI_SWEEPS = 12
TREE_MIN_LEAVES = 2048
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
INF = float("inf")


# ---- nearest neighbours --------------------------------------------------------------------------------------------------
def nn_search(queries, targets, max_distance=INF, chunk=256):
    """-> (j int32, -1: none; d2 float32, +inf: none).  d2 = (dx*dx + dy*dy) + dz*dz in float32, least d2 over the finite
    targets, ties to the lowest j (np.argmin returns the first least element); kept iff (double)d2 <= D * D."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    valid = np.flatnonzero(np.isfinite(t).all(axis=1))
    tv = t[valid]
    j = np.full(len(q), -1, np.int32)
    d2 = np.full(len(q), np.inf, np.float32)
    if len(tv) == 0:
        return j, d2
    bound = float(max_distance) * float(max_distance)
    live = np.isfinite(q).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(q), chunk):
            qa = q[a:a + chunk]
            dx = qa[:, None, 0] - tv[None, :, 0]
            dy = qa[:, None, 1] - tv[None, :, 1]
            dz = qa[:, None, 2] - tv[None, :, 2]
            s = (dx * dx + dy * dy) + dz * dz
            assert s.dtype == np.float32
            k = np.argmin(np.where(np.isnan(s), np.inf, s), axis=1)  # (NaN only beside a non-finite query)
            best = s[np.arange(len(qa)), k]
            keep = live[a:a + chunk] & (best.astype(np.float64) <= bound)
            j[a:a + chunk] = np.where(keep, valid[k], -1)
            d2[a:a + chunk] = np.where(keep, best, np.inf)
    return j, d2


# ---- the fixed tree ----------------------------------------------------------------------------------------------------------
def tree_sum(values):
    """Columns of a float64 array summed over axis 0: padded with +0.0 to max(2048, the next power of two) leaves, adjacent
    pairs added level by level."""
    v = np.asarray(values, np.float64)
    v = v.reshape(len(v), -1)
    leaves = TREE_MIN_LEAVES
    while leaves < len(v):
        leaves *= 2
    a = np.zeros((leaves, v.shape[1]), np.float64)
    a[:len(v)] = v
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def correspondence_sums(points, targets, j, d2):
    """-> (sums (16,) float64: Sp, Sq, Spq row-major, Sd; n)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    has = j >= 0
    q = np.asarray(targets, np.float32).astype(np.float64)[np.where(has, j, 0)]
    leaves = np.zeros((len(p), 16), np.float64)
    leaves[:, 0:3] = p
    leaves[:, 3:6] = q
    leaves[:, 6:15] = (p[:, :, None] * q[:, None, :]).reshape(-1, 9)
    leaves[:, 15] = np.where(has, d2, 0).astype(np.float64)
    leaves[~has] = 0.0
    return tree_sum(leaves) if len(p) else np.zeros(16), int(has.sum())


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def solve(sums, n):
    """Horn's quaternion by cyclic Jacobi, in Python floats -> (R 3x3 list, t list)"""
    S = [float(v) for v in sums]
    dn = float(n)
    cp = [S[a] / dn for a in range(3)]
    cq = [S[3 + a] / dn for a in range(3)]
    H = [[S[6 + 3 * a + b] - (S[a] * S[3 + b]) / dn for b in range(3)] for a in range(3)]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (H[0][0] + H[1][1]) + H[2][2]
    A[0][1] = H[1][2] - H[2][1]
    A[0][2] = H[2][0] - H[0][2]
    A[0][3] = H[0][1] - H[1][0]
    A[1][1] = (H[0][0] - H[1][1]) - H[2][2]
    A[1][2] = H[0][1] + H[1][0]
    A[1][3] = H[2][0] + H[0][2]
    A[2][2] = (H[1][1] - H[0][0]) - H[2][2]
    A[2][3] = H[1][2] + H[2][1]
    A[3][3] = (H[2][2] - H[0][0]) - H[1][1]
    for r in range(4):
        for c in range(r):
            A[r][c] = A[c][r]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(JACOBI_SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(tt * tt + 1.0)
                s = tt * c
                A[p][p] = A[p][p] - tt * apq
                A[q][q] = A[q][q] + tt * apq
                A[p][q] = A[q][p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        A[r][p] = A[p][r] = c * arp - s * arq
                        A[r][q] = A[q][r] = s * arp + c * arq
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - s * vrq
                    V[r][q] = s * vrp + c * vrq
    best = 0
    for c in range(1, 4):
        if A[c][c] > A[best][best]:
            best = c
    w, x, y, z = V[0][best], V[1][best], V[2][best], V[3][best]
    norm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]
    t = [cq[a] - ((R[a][0] * cp[0] + R[a][1] * cp[1]) + R[a][2] * cp[2]) for a in range(3)]
    return R, t


def transform_points(R, t, points):
    """(float)(((r0*x + r1*y) + r2*z) + t) in double from float32 points"""
    p = np.asarray(points, np.float32).astype(np.float64)
    out = np.empty_like(p)
    for a in range(3):
        out[:, a] = ((R[a][0] * p[:, 0] + R[a][1] * p[:, 1]) + R[a][2] * p[:, 2]) + t[a]
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


def compose(R, t, T):
    """[R t; 0 0 0 1] T, each entry ((m0*t0 + m1*t1) + m2*t2), the translation column + t"""
    out = [[0.0] * 4 for _ in range(4)]
    for a in range(3):
        for b in range(4):
            v = (R[a][0] * T[0][b] + R[a][1] * T[1][b]) + R[a][2] * T[2][b]
            out[a][b] = v + t[a] if b == 3 else v
    out[3] = [0.0, 0.0, 0.0, 1.0]
    return out


# ---- convergence -------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(max_correspondence_distance=30.0, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6,
                rotation_epsilon=1e-5, relative_mse_epsilon=1e-5, maximum_iterations=100, min_correspondences=3)


def options(**overrides):
    o = dict(DEFAULTS)
    o.update(overrides)
    return o


def decide(k, R, t, mse, previous_mse, o):
    """The header's four tests in their order -> reason (NOT_CONVERGED: go on)"""
    if k >= o["maximum_iterations"]:
        return ITERATIONS
    cosine = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1.0)
    translation_sq = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    if cosine >= 1.0 - o["rotation_epsilon"] and translation_sq <= o["transformation_epsilon"]:
        return TRANSFORM
    change = abs(mse - previous_mse)
    if change < o["euclidean_fitness_epsilon"]:
        return ABS_MSE
    with np.errstate(all="ignore"):  # IEEE: inf / inf and 0 / 0 are NaN, and NaN < x is false
        ratio = float(np.float64(change) / np.float64(previous_mse))
    if ratio < o["relative_mse_epsilon"]:
        return REL_MSE
    return NOT_CONVERGED


def align(source, target, guess=None, o=None, search=None):
    """dliom_icp_align's result as a dict, with the final points under "aligned".  search: another exact search in
    nn_search's place (tools/icp_bench.py: a kd-tree that is checked against the float rule)"""
    nn_search = search or globals()["nn_search"]
    o = o or options()
    T = [[float(v) for v in row] for row in (np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4))]
    p = transform_points([row[:3] for row in T[:3]], [row[3] for row in T[:3]], source)
    res = dict(converged=0, reason=NOT_CONVERGED, iterations=0, correspondences=0, mse=INF)
    previous = INF
    k = 0
    while True:
        k += 1
        j, d2 = nn_search(p, target, o["max_correspondence_distance"])
        sums, n = correspondence_sums(p, target, j, d2)
        res["correspondences"] = n
        if n < o["min_correspondences"]:
            res["reason"] = NO_CORRESPONDENCES
            break
        R, t = solve(sums, n)
        T = compose(R, t, T)
        mse = float(sums[15]) / float(n)
        res["mse"], res["iterations"] = mse, k
        reason = decide(k, R, t, mse, previous, o)
        previous = mse
        p = transform_points(R, t, p)
        if reason != NOT_CONVERGED:
            res["converged"], res["reason"] = 1, reason
            break
    j, d2 = nn_search(p, target, INF)
    has = j >= 0
    res["fitness_count"] = int(has.sum())
    res["fitness_score"] = float(tree_sum(np.where(has, d2, 0).astype(np.float64))[0]) / res["fitness_count"] if has.any() else float("nan")
    res["transform"] = np.array(T, np.float64)
    res["aligned"] = p
    return res


def step(points, target, o=None):
    o = o or options()
    j, d2 = nn_search(points, target, o["max_correspondence_distance"])
    sums, n = correspondence_sums(points, target, j, d2)
    R, t = (solve(sums, n) if n >= o["min_correspondences"] else ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [0.0] * 3))
    return dict(j=j, d2=d2, sums=sums, n=n, R=np.array(R), t=np.array(t))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
IDENTITY7 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def pose_matrix(pose7):
    T = np.eye(4)
    T[:3, :3] = synth.quat_to_matrix(pose7[3:])
    T[:3, 3] = pose7[:3]
    return T


_CACHE = {}


def ground_scan(t=0.30):
    """The `ground` scene's 16 x 128 scan at the corkscrew's trajectory_pose(t), sensor frame (1753 points at t = 0.30)"""
    if t not in _CACHE:
        with synth.scene("ground", trajectory=False):
            _CACHE[t] = synth.scan(synth.trajectory_pose(t), 16, 128)[0]
        _CACHE[t].setflags(write=False)
    return _CACHE[t]


def moved_copy(max_translation=0.3, max_angle_deg=2.0, seed=3):
    """-> (source: every other point of ground_scan() moved by perturb_pose(identity, ...), target, the motion 4x4)"""
    target = ground_scan()
    motion = synth.perturb_pose(IDENTITY7, max_translation, max_angle_deg, seed=seed)
    return synth.transform_points(motion, target[::2]), target, pose_matrix(motion)


def kabsch(p, q):
    """numpy's SVD-Kabsch on paired float64 points -> (R, t): the independent solve of the host test"""
    cp, cq = p.mean(axis=0), q.mean(axis=0)
    U, _, Vt = np.linalg.svd((p - cp).T @ (q - cq))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cq - R @ cp
