"""numpy model of the IMU-LiDAR initialisation's arithmetic as include/dliom.h states it ("IMU-LiDAR initialisation"):
FROM TWO VECTORS with its written rule for nearly opposite vectors, and InitializeStatic.  Python floats are IEEE doubles
and every operation below is one rounded operation, in the header's order, so the library can be compared bit for bit."""
import math

import numpy as np


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def normalized(v):
    n = math.sqrt(dot(v, v))
    return [v[0] / n, v[1] / n, v[2] / n]


def from_two_vectors(a, b):
    """-> (w, x, y, z), and whether the nearly-opposite rule was taken"""
    v0, v1 = normalized([float(x) for x in a]), normalized([float(x) for x in b])
    c = dot(v1, v0)
    if c < -1.0 + 1e-12:
        m = [abs(x) for x in v0]
        k = 0
        if m[1] < m[k]:
            k = 1
        if m[2] < m[k]:
            k = 2
        axis = normalized(cross(v0, [1.0 if k == 0 else 0.0, 1.0 if k == 1 else 0.0, 1.0 if k == 2 else 0.0]))
        return [0.0] + axis, True
    axis = cross(v0, v1)
    s = math.sqrt((1.0 + c) * 2.0)
    invs = 1.0 / s
    return [s * 0.5, axis[0] * invs, axis[1] * invs, axis[2] * invs], False


def rotation_of(q):
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def static_initialization(acc, gyr, gravity_norm):
    """InitializeStatic -> dict(R, ba, bg, P, V, opposite)"""
    acc, gyr = np.asarray(acc, np.float64).reshape(-1, 3), np.asarray(gyr, np.float64).reshape(-1, 3)
    acc_sum, gyr_sum = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for a, g in zip(acc.tolist(), gyr.tolist()):
        for k in range(3):
            acc_sum[k] += a[k]
            gyr_sum[k] += g[k]
    count = float(len(acc))
    acc_mean = [s / count for s in acc_sum]
    g_vec = [0.0, 0.0, -float(gravity_norm)]
    q, opposite = from_two_vectors(acc_mean, [-g_vec[0], -g_vec[1], -g_vec[2]])
    R = rotation_of(q)
    ba = [((float(R[0, a]) * g_vec[0] + float(R[1, a]) * g_vec[1]) + float(R[2, a]) * g_vec[2]) + acc_mean[a] for a in range(3)]
    return {"R": R, "ba": np.array(ba), "bg": np.array([s / count for s in gyr_sum]), "P": np.zeros(3), "V": np.zeros(3),
            "opposite": opposite, "acc_mean": np.array(acc_mean)}


# ---- Initializer::Initialization and AlignWithWorld -------------------------------------------------------------------------
OK, NO_EXCITATION, TOO_FEW_FRAMES, GRAVITY_NORM, SINGULAR = range(5)


def tangent_basis(g0):
    a = np.array(normalized(list(g0)))
    tmp = np.array([0.0, 0.0, 1.0])
    if (a == tmp).all():
        tmp = np.array([1.0, 0.0, 0.0])
    b = np.array(normalized(list(tmp - a * dot(a, tmp))))
    return np.stack([b, np.array(cross(a, b))], axis=1)  # 3 x 2


def _assemble(frames, tlb, basis, g0, A, b):
    """Adds every pair's M^T M and M^T r (dliom.h) to A and b.  frames: (pose7, preintegration or None)"""
    G = basis.shape[1]
    n_state = len(b)
    tail = n_state - G
    R = [rotation_of(f[0][3:]) for f in frames]
    for i in range(len(frames) - 1):
        pre = frames[i + 1][1]
        if pre is None:
            continue
        dt = float(pre["sum_dt"])
        RiT = R[i].T
        RiTRj = RiT @ R[i + 1]
        M = np.zeros((6, 6 + G))
        M[0:3, 0:3] = -dt * np.eye(3)
        M[0:3, 6:] = (RiT @ basis) * (dt * dt / 2.0)
        M[3:6, 0:3] = -np.eye(3)
        M[3:6, 3:6] = RiTRj
        M[3:6, 6:] = (RiT @ basis) * dt
        apart = RiT @ (np.asarray(frames[i + 1][0][:3], float) - np.asarray(frames[i][0][:3], float))
        top = np.asarray(pre["delta_p"], float) + RiTRj @ tlb - tlb
        bottom = np.asarray(pre["delta_v"], float).copy()
        if g0 is not None:
            top = top - (RiT @ g0) * (dt * dt / 2.0)
            bottom = bottom - (RiT @ g0) * dt
        r = np.concatenate([top - apart, bottom])
        cols = list(range(3 * i, 3 * i + 6)) + list(range(tail, n_state))
        A[np.ix_(cols, cols)] += M.T @ M
        b[cols] += M.T @ r


def _solve(A, b, solves):
    """np.linalg.solve, with the bound of the solve noted: 64 * cond(A) * 2^-52 * |x|"""
    x = np.linalg.solve(A, b)
    solves.append({"cond": float(np.linalg.cond(A)), "x_norm": float(np.linalg.norm(x)),
                   "bound": 64.0 * float(np.linalg.cond(A)) * 2.0 ** -52 * float(np.linalg.norm(x))})
    return x


def initialization(frames, transform_lb, g_norm):
    """-> dict(outcome, velocities (n, 3), gravity, solves: cond, |x| and bound of each solve, approximate_norm_gap)"""
    n = len(frames)
    out = {"outcome": TOO_FEW_FRAMES, "velocities": np.zeros((n, 3)), "gravity": np.zeros(3), "solves": []}
    if n < 7:
        return out
    tlb = np.asarray(transform_lb[:3], float)
    A, b = np.zeros((3 * n + 3, 3 * n + 3)), np.zeros(3 * n + 3)
    _assemble(frames, tlb, np.eye(3), None, A, b)
    A *= 1000.0
    b *= 1000.0
    try:
        g = _solve(A, b, out["solves"])[-3:]
    except np.linalg.LinAlgError:
        out["outcome"] = SINGULAR
        return out
    out["gravity"] = g
    out["approximate_norm_gap"] = abs(np.linalg.norm(g) - g_norm)
    if not out["approximate_norm_gap"] < 1.0:
        out["outcome"] = GRAVITY_NORM
        return out
    A, b = np.zeros((3 * n + 2, 3 * n + 2)), np.zeros(3 * n + 2)  # zeroed once: not between the passes
    g0 = np.array(normalized(list(g))) * g_norm
    for _ in range(4):
        basis = tangent_basis(g0)
        _assemble(frames, tlb, basis, g0, A, b)
        A *= 1000.0
        b *= 1000.0
        x = _solve(A, b, out["solves"])
        g0 = np.array(normalized(list(g0 + basis @ x[-2:]))) * g_norm
    out["gravity"], out["velocities"] = g0, x[:3 * n].reshape(n, 3).copy()
    out["outcome"] = OK if abs(np.linalg.norm(g0) - g_norm) < 0.2 else GRAVITY_NORM
    return out


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def excitation_of(frames):
    later = len(frames) - 1
    t = [np.asarray(f[1]["delta_v"], float) / float(f[1]["sum_dt"]) for f in frames[1:] if f[1] is not None]
    mean = np.sum(t, axis=0) / later if t else np.zeros(3)
    return float(np.sqrt(sum(float((v - mean) @ (v - mean)) for v in t) / later))


def align_with_world(frames, transform_lb, g_norm):
    out = {"excitation": excitation_of(frames), "outcome": NO_EXCITATION, "solves": []}
    if out["excitation"] < 0.25:
        return out
    init = initialization(frames, transform_lb, g_norm)
    out.update(outcome=init["outcome"], solves=init["solves"], gravity_in_laser=init["gravity"], local_velocities=init["velocities"],
               approximate_norm_gap=init.get("approximate_norm_gap"))
    if init["outcome"] != OK:
        return out
    lb = np.asarray(transform_lb, float)
    q, _ = from_two_vectors(normalized(list(-init["gravity"])), [0.0, 0.0, -1.0])
    Rw = rotation_of(q)
    P, R, V = [], [], []
    for (pose, _), v in zip(frames, init["velocities"]):
        pose = np.asarray(pose, float)
        qq = quat_mul(pose[3:], lb[3:])
        Ri = rotation_of(qq / np.linalg.norm(qq))
        P.append(Rw @ (rotation_of(pose[3:]) @ lb[:3] + pose[:3]))
        R.append(Rw @ Ri)
        V.append(Rw @ (Ri @ v))
    out.update(P=np.array(P), R=np.array(R), V=np.array(V), world_rotation=Rw)
    return out
