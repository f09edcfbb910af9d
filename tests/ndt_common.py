"""The CPU model of include/dliom.h "scan alignment by NDT", operation for operation: numpy float32 for cell indices and
the neighbour test, numpy float64 element-wise operations for the per-point values (one rounding an operation, like the
device), Python floats and `math` (the host's libm) for the per-cell step, the pose, the constants, the pseudo-inverse and
the step length.  The GPU tests compare bits against it; tests/test_ndt_host.py checks it against independent means."""
import math

import numpy as np

import icp_common as ic
from icp_common import tree_sum  # noqa: F401  (ICP's fixed tree over the source index)

JACOBI_SWEEPS, PINV_SWEEPS, HALF = 8, 12, 1 << 20
STEP_CLAMPED, STEP_MORE_THUENTE = 0, 1
NOT_CONVERGED, ITERATIONS, EPSILON, ZERO_STEP = range(4)
EVAL_GRADIENT, EVAL_ALL, EVAL_HESSIAN = range(3)
DEFAULTS = dict(resolution=1.0, step_size=0.1, transformation_epsilon=0.01, outlier_ratio=0.55, maximum_iterations=35,
                min_points_per_voxel=6, step_mode=STEP_CLAMPED)
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
HESSIAN_OF = {(3, 3): 0, (3, 4): 1, (3, 5): 2, (4, 4): 3, (4, 5): 4, (5, 5): 5}


def options(**overrides):
    o = dict(DEFAULTS)
    o.update(overrides)
    return o


# ---- target cells --------------------------------------------------------------------------------------------------------------
def cell_indices(points, resolution):
    """-> (float32 (n, 3) floors, bool (n,) kept): floor(x * inv) in float32, inv = 1.0f / (float)resolution"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    inv = np.float32(1.0) / np.float32(resolution)
    with np.errstate(all="ignore"):
        f = np.floor(p * inv)
    assert f.dtype == np.float32
    return f, np.isfinite(p).all(axis=1)


def pow2_tree_sum(values):
    """Columns summed over axis 0: padded with +0.0 to the next power of two, adjacent pairs added level by level"""
    v = np.asarray(values, np.float64).reshape(len(values), -1)
    leaves = 1
    while leaves < len(v):
        leaves *= 2
    a = np.zeros((leaves, v.shape[1]), np.float64)
    a[:len(v)] = v
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def jacobi(A, sweeps):
    """Cyclic Jacobi with ICP's rotation rule on a symmetric matrix (list of lists, changed in place) -> V"""
    n = len(A)
    V = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
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
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        A[r][p] = A[p][r] = c * arp - s * arq
                        A[r][q] = A[q][r] = s * arp + c * arq
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - s * vrq
                    V[r][q] = s * vrp + c * vrq
    return V


def eigen3(C):
    """-> (ascending eigenvalues, V with the matching columns' indices): the header's fixed Jacobi and stable sort"""
    A = [list(map(float, row)) for row in C]
    V = jacobi(A, JACOBI_SWEEPS)
    order = sorted(range(3), key=lambda k: A[k][k])  # stable
    return [A[k][k] for k in order], V, order


def div(a, b):
    """IEEE double division (Python raises where IEEE gives inf or NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def finish_cell(S, n, min_points):
    """-> (mean list, icov list of 6, valid)"""
    S = [float(v) for v in S]
    dn = float(n)
    mean = [S[a] / dn for a in range(3)]
    zeros = [0.0] * 6
    if n < min_points:
        return mean, zeros, False
    at = [[3, 4, 5], [4, 6, 7], [5, 7, 8]]
    C = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            C[a][b] = C[b][a] = ((S[at[a][b]] - 2.0 * (S[a] * mean[b])) / dn + mean[a] * mean[b]) * ((dn - 1.0) / dn)
    lam, V, order = eigen3(C)
    if not (lam[0] >= 0.0 and lam[1] >= 0.0 and lam[2] > 0.0):
        return mean, zeros, False
    least = 0.01 * lam[2]
    lam = [max(lam[0], least) if lam[0] < least else lam[0], max(lam[1], least) if lam[1] < least else lam[1], lam[2]]
    icov = []
    for a in range(3):
        for b in range(a, 3):
            icov.append((div(V[a][order[0]] * V[b][order[0]], lam[0]) + div(V[a][order[1]] * V[b][order[1]], lam[1])) +
                        div(V[a][order[2]] * V[b][order[2]], lam[2]))
    if not all(math.isfinite(v) for v in icov):
        return mean, zeros, False
    return mean, icov, True


def key_of(ix, iy, iz):
    return ((np.asarray(iz, np.int64) + HALF) << 42) | ((np.asarray(iy, np.int64) + HALF) << 21) | (np.asarray(ix, np.int64) + HALF)


def build_cells(target, o=None):
    """-> dict(index (m, 3) int32, n, valid, mean (m, 3), icov (m, 6), sums (m, 9)) in key order (z, y, x), plus the valid
    cells' sorted keys / mean / icov under "valid_keys", "valid_mean", "valid_icov"."""
    o = o or options()
    p = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    f, finite = cell_indices(p, o["resolution"])
    with np.errstate(invalid="ignore"):
        kept = finite & (f >= -float(HALF)).all(axis=1) & (f < float(HALF)).all(axis=1)
    which = np.flatnonzero(kept)
    idx = f[which].astype(np.int64)
    keys = key_of(idx[:, 0], idx[:, 1], idx[:, 2])
    order = np.argsort(keys, kind="stable")
    sk, si = keys[order], which[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if len(sk) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(sk)]
    m = len(starts)
    out = dict(index=np.zeros((m, 3), np.int32), n=np.zeros(m, np.int64), valid=np.zeros(m, bool), mean=np.zeros((m, 3)),
               icov=np.zeros((m, 6)), sums=np.zeros((m, 9)), keys=sk[starts] if m else np.zeros(0, np.int64))
    d = p.astype(np.float64)
    for c in range(m):
        members = si[starts[c]:ends[c]]
        x = d[members]
        leaves = np.stack([x[:, 0], x[:, 1], x[:, 2], x[:, 0] * x[:, 0], x[:, 0] * x[:, 1], x[:, 0] * x[:, 2], x[:, 1] * x[:, 1],
                           x[:, 1] * x[:, 2], x[:, 2] * x[:, 2]], axis=1)
        S = pow2_tree_sum(leaves)
        mean, icov, valid = finish_cell(S, len(members), o["min_points_per_voxel"])
        k = int(out["keys"][c])
        out["index"][c] = [(k & 0x1fffff) - HALF, ((k >> 21) & 0x1fffff) - HALF, ((k >> 42) & 0x1fffff) - HALF]
        out["n"][c], out["valid"][c], out["mean"][c], out["icov"][c], out["sums"][c] = len(members), valid, mean, icov, S
    v = out["valid"]
    out["valid_keys"], out["valid_mean"], out["valid_icov"] = out["keys"][v], out["mean"][v], out["icov"][v]
    out["kept_points"] = int(kept.sum())
    return out


# ---- neighbours ----------------------------------------------------------------------------------------------------------------
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def neighbours(cells, queries, resolution):
    """-> list over the 27 offsets, in the header's order, of (query indices, valid-cell indices): the neighbour pairs"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    f, finite = cell_indices(q, resolution)
    with np.errstate(invalid="ignore"):
        live = finite & (f >= -float(HALF + 1)).all(axis=1) & (f <= float(HALF)).all(axis=1)
    out = []
    vk = cells["valid_keys"]
    if len(vk) == 0 or not live.any():
        return [(np.zeros(0, np.int64), np.zeros(0, np.int64))] * 27
    who = np.flatnonzero(live)
    base = f[who].astype(np.int64)
    r2 = np.float32(resolution) * np.float32(resolution)
    m32 = cells["valid_mean"].astype(np.float32)
    for dx, dy, dz in OFFSETS:
        c = base + np.array([dx, dy, dz])
        inside = ((c >= -HALF) & (c < HALF)).all(axis=1)
        k = key_of(c[:, 0], c[:, 1], c[:, 2])
        at = np.searchsorted(vk, k)
        hit = inside & (at < len(vk))
        hit[hit] = vk[at[hit]] == k[hit]
        qi, ci = who[hit], at[hit]
        d = q[qi] - m32[ci]
        with np.errstate(over="ignore"):
            near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
        out.append((qi[near], ci[near]))
    return out


# ---- constants, pose, derivatives ----------------------------------------------------------------------------------------------
def constants(o):
    """-> (d1, d2)"""
    res, ratio = float(o["resolution"]), float(o["outlier_ratio"])
    c1 = 10.0 * (1.0 - ratio)
    c2 = ratio / ((res * res) * res)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def pose_terms(p):
    """-> (R 3x3, t, J {(angle, component): row}, H {(which, component): row}) as Python floats"""
    sa, ca, sb, cb, sc, cc = math.sin(p[3]), math.cos(p[3]), math.sin(p[4]), math.cos(p[4]), math.sin(p[5]), math.cos(p[5])
    R = [[cb * cc, -(cb * sc), sb],
         [ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -(sa * cb)],
         [sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb]]
    J = {(0, 1): (-(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, -(ca * cb)),
         (0, 2): (ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -(sa * cb)),
         (1, 0): (-(sb * cc), sb * sc, cb),
         (1, 1): (sa * cb * cc, -(sa * cb * sc), sa * sb),
         (1, 2): (-(ca * cb * cc), ca * cb * sc, -(ca * sb)),
         (2, 0): (-(cb * sc), -(cb * cc), 0.0),
         (2, 1): (ca * cc - sa * sb * sc, -(ca * sc) - sa * sb * cc, 0.0),
         (2, 2): (sa * cc + ca * sb * sc, -(sa * sc) + ca * sb * cc, 0.0)}
    H = {(0, 1): (-(ca * sc) - sa * sb * cc, -(ca * cc) + sa * sb * sc, sa * cb),
         (0, 2): (-(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, -(ca * cb)),
         (1, 1): (ca * cb * cc, -(ca * cb * sc), ca * sb),
         (1, 2): (sa * cb * cc, -(sa * cb * sc), sa * sb),
         (2, 1): (-(sa * cc) - ca * sb * sc, sa * sc - ca * sb * cc, 0.0),
         (2, 2): (ca * cc - sa * sb * sc, -(ca * sc) - sa * sb * cc, 0.0),
         (3, 0): (-(cb * cc), cb * sc, -sb),
         (3, 1): (-(sa * sb * cc), sa * sb * sc, sa * cb),
         (3, 2): (ca * sb * cc, -(ca * sb * sc), -(ca * cb)),
         (4, 0): (sb * sc, sb * cc, 0.0),
         (4, 1): (-(sa * cb * sc), -(sa * cb * cc), 0.0),
         (4, 2): (ca * cb * sc, ca * cb * cc, 0.0),
         (5, 0): (-(cb * cc), cb * sc, 0.0),
         (5, 1): (-(ca * sc) - sa * sb * cc, -(ca * cc) + sa * sb * sc, 0.0),
         (5, 2): (-(sa * sc) + ca * sb * cc, -(sa * cc) - ca * sb * sc, 0.0)}
    return R, [float(p[0]), float(p[1]), float(p[2])], J, H


def pose_of_guess(guess):
    g = np.asarray(guess, np.float64).reshape(4, 4)
    R = [[float(v) for v in row[:3]] for row in g[:3]]
    return [float(g[0, 3]), float(g[1, 3]), float(g[2, 3]), math.atan2(-R[1][2], R[2][2]),
            math.atan2(R[0][2], math.sqrt(R[0][0] * R[0][0] + R[0][1] * R[0][1])), math.atan2(-R[0][1], R[0][0])]


def transform_of(p):
    R, t, _, _ = pose_terms(p)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def point_vectors(x, rows, count):
    """(n, count, 3): component r of vector a is the row (a, r) dotted with x as (k0*x0 + k1*x1) + k2*x2; +0.0 where unlisted"""
    out = np.zeros((len(x), count, 3))
    with np.errstate(all="ignore"):  # (a source point may be non-finite: it has no neighbours, its vectors are not used)
        for (a, r), k in rows.items():
            out[:, a, r] = (k[0] * x[:, 0] + k[1] * x[:, 1]) + k[2] * x[:, 2]
    return out


# ---- E ------------------------------------------------------------------------------------------------------------------------
EXP_COEFFICIENTS = [1.0 / math.factorial(n) for n in range(14)]


def E(u):
    u = np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        k = np.rint(u * float.fromhex("0x1.71547652b82fep+0"))
        r = (u - k * float.fromhex("0x1.62e42fee00000p-1")) - k * float.fromhex("0x1.a39ef35793c76p-33")
        p = np.full_like(u, EXP_COEFFICIENTS[13])
        for n in range(12, -1, -1):
            p = p * r + EXP_COEFFICIENTS[n]
        middle = np.isfinite(k) & (np.abs(k) < 1100)
        v = np.ldexp(p, np.where(middle, k, 0).astype(np.int64))
    v = np.where(u > 708.0, np.inf, v)
    v = np.where(u != u, u, v)
    return np.where(u < -708.0, 0.0, v)


# ---- evaluation --------------------------------------------------------------------------------------------------------------
def dot3(m, v):
    """rows (m[..., r, 0]*v0 + m[..., r, 1]*v1) + m[..., r, 2]*v2 of a batch of symmetric 3x3 and vectors -> (n, 3)"""
    return (m[:, :, 0] * v[:, None, 0] + m[:, :, 1] * v[:, None, 1]) + m[:, :, 2] * v[:, None, 2]


def vdot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def full_icov(icov6):
    m = np.empty((len(icov6), 3, 3))
    at = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    for a in range(3):
        for b in range(3):
            m[:, a, b] = icov6[:, at[a][b]]
    return m


def point_values(cells, source, p, o, what=EVAL_ALL):
    """-> (values (n, 28): score, g, H upper row-major, zeros where `what` leaves them out; pairs (n,))"""
    d1, d2 = constants(o)
    R, t, Jrows, Hrows = pose_terms(p)
    src = np.ascontiguousarray(source, np.float32).reshape(-1, 3)
    x = src.astype(np.float64)
    with np.errstate(all="ignore"):
        q = ic.transform_points(R, t, src)
    Jv, Hv = point_vectors(x, Jrows, 3), point_vectors(x, Hrows, 6)
    values, pairs = np.zeros((len(x), 28)), np.zeros(len(x), np.int64)
    G, Hs = what != EVAL_HESSIAN, what != EVAL_GRADIENT
    with np.errstate(all="ignore"):
        for qi, ci in neighbours(cells, q, o["resolution"]):
            if len(qi) == 0:
                continue
            pairs[qi] += 1
            icov = full_icov(cells["valid_icov"][ci])
            xt = q[qi].astype(np.float64) - cells["valid_mean"][ci]
            w = dot3(icov, xt)
            qq = vdot(xt, w)
            e = E(-(d2 * qq) * 0.5)
            f = d2 * e
            ok = ~((f > 1.0) | (f < 0.0) | (f != f))
            qi, icov, xt, e, f = qi[ok], icov[ok], xt[ok], e[ok], f[ok]
            if G:
                values[qi, 0] += -d1 * e
            f = f * d1
            cJ = [icov[:, :, a] if a < 3 else dot3(icov, Jv[qi, a - 3]) for a in range(6)]
            u = [vdot(xt, cJ[a]) for a in range(6)]
            if G:
                for a in range(6):
                    values[qi, 1 + a] += u[a] * f
            if Hs:
                for slot, (a, b) in enumerate(UPPER):
                    h = vdot(xt, dot3(icov, Hv[qi, HESSIAN_OF[(a, b)]])) if a >= 3 else 0.0
                    k = cJ[a][:, b] if b < 3 else vdot(Jv[qi, b - 3], cJ[a])
                    values[qi, 7 + slot] += f * ((((-d2) * u[a]) * u[b] + h) + k)
    return values, pairs


def evaluate(cells, source, p, o=None, what=EVAL_ALL):
    """-> dict(score, gradient (6,), hessian (6, 6), pairs)"""
    o = o or options()
    values, pairs = point_values(cells, source, p, o, what)
    sums = tree_sum(values) if len(values) else np.zeros(28)
    H = np.zeros((6, 6))
    for slot, (a, b) in enumerate(UPPER):
        H[a, b] = H[b, a] = sums[7 + slot]
    return dict(score=float(sums[0]), gradient=sums[1:7].copy(), hessian=H, pairs=int(pairs.sum()))


# ---- alignment ---------------------------------------------------------------------------------------------------------------
def pinv6(H):
    """The header's pseudo-inverse as a matrix (for the host test); newton_step applies the same steps to g"""
    return np.array([[-v for v in newton_step(H, [1.0 if r == c else 0.0 for r in range(6)])] for c in range(6)]).T


def newton_step(H, g):
    A = [[float(v) for v in row] for row in np.asarray(H)]
    V = jacobi(A, PINV_SWEEPS)
    largest = 0.0
    for k in range(6):
        if abs(A[k][k]) > largest:
            largest = abs(A[k][k])
    floor = 6.0 * 2.0 ** -52 * largest
    z = []
    for k in range(6):
        y = 0.0
        for r in range(6):
            y = y + V[r][k] * float(g[r])
        z.append(div(y, A[k][k]) if abs(A[k][k]) > floor else 0.0)
    delta = []
    for r in range(6):
        v = 0.0
        for k in range(6):
            v = v + V[r][k] * z[k]
        delta.append(-v)
    return delta


def min_of(a, b):
    return b if b < a else a


def max_of(a, b):
    return b if a < b else a


def fsqrt(v):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))


def mt_trial(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
    if f_t > f_l:
        z = (div(3.0 * (f_t - f_l), a_t - a_l) - g_t) - g_l
        w = fsqrt(z * z - g_t * g_l)
        a_c = a_l + div((a_t - a_l) * ((w - g_l) - z), (g_t - g_l) + 2.0 * w)
        a_q = a_l - div(0.5 * (a_l - a_t) * g_l, g_l - div(f_l - f_t, a_l - a_t))
        return a_c if abs(a_c - a_l) < abs(a_q - a_l) else 0.5 * (a_q + a_c)
    if g_t * g_l < 0.0:
        z = (div(3.0 * (f_t - f_l), a_t - a_l) - g_t) - g_l
        w = fsqrt(z * z - g_t * g_l)
        a_c = a_l + div((a_t - a_l) * ((w - g_l) - z), (g_t - g_l) + 2.0 * w)
        a_s = a_l - div(a_l - a_t, g_l - g_t) * g_l
        return a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s
    if abs(g_t) <= abs(g_l):
        z = (div(3.0 * (f_t - f_l), a_t - a_l) - g_t) - g_l
        w = fsqrt(z * z - g_t * g_l)
        a_c = a_l + div((a_t - a_l) * ((w - g_l) - z), (g_t - g_l) + 2.0 * w)
        a_s = a_l - div(a_l - a_t, g_l - g_t) * g_l
        nxt = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
        bound = a_t + 0.66 * (a_u - a_t)
        return min_of(bound, nxt) if a_t > a_l else max_of(bound, nxt)
    z = (div(3.0 * (f_t - f_u), a_t - a_u) - g_t) - g_u
    w = fsqrt(z * z - g_t * g_u)
    return a_u + div((a_t - a_u) * ((w - g_u) - z), (g_t - g_u) + 2.0 * w)


def mt_update(s, a_t, f_t, g_t):
    """s: dict a_l f_l g_l a_u f_u g_u, changed in place -> converged"""
    if f_t > s["f_l"]:
        s["a_u"], s["f_u"], s["g_u"] = a_t, f_t, g_t
        return False
    if g_t * (s["a_l"] - a_t) > 0.0:
        s["a_l"], s["f_l"], s["g_l"] = a_t, f_t, g_t
        return False
    if g_t * (s["a_l"] - a_t) < 0.0:
        s["a_u"], s["f_u"], s["g_u"] = s["a_l"], s["f_l"], s["g_l"]
        s["a_l"], s["f_l"], s["g_l"] = a_t, f_t, g_t
        return False
    return True


def dot6(a, b):
    v = 0.0
    for r in range(6):
        v = v + float(a[r]) * float(b[r])
    return v


class Run:
    """The evaluations of one alignment, counted"""

    def __init__(self, cells, source, o):
        self.cells, self.source, self.o = cells, source, o
        self.with_hessian = self.without_hessian = 0

    def evaluate(self, p, what, sums):
        if what == EVAL_GRADIENT:
            self.without_hessian += 1
        else:
            self.with_hessian += 1
        e = evaluate(self.cells, self.source, p, self.o, what)
        if what != EVAL_HESSIAN:
            sums["score"], sums["gradient"] = e["score"], e["gradient"]
        if what != EVAL_GRADIENT:
            sums["hessian"] = e["hessian"]
        sums["pairs"] = e["pairs"]


def step_length(run, p, direction, step_init, o, sums):
    """-> a; `direction` (a list) may be negated in place, `sums` becomes the last evaluation's"""
    step_max, step_min = float(o["step_size"]), float(o["transformation_epsilon"]) / 2.0
    phi0 = -sums["score"]
    dphi0 = -dot6(sums["gradient"], direction)
    if dphi0 == 0.0:
        return 0.0
    if dphi0 > 0.0:
        dphi0 = -dphi0
        for r in range(6):
            direction[r] = -direction[r]
    a_t = max_of(min_of(step_init, step_max), step_min)
    x = [p[r] + direction[r] * a_t for r in range(6)]
    run.evaluate(x, EVAL_ALL, sums)
    if o["step_mode"] == STEP_CLAMPED:
        return a_t
    mu, nu = 1e-4, 0.9
    s = dict(a_l=0.0, a_u=0.0, f_l=0.0, f_u=0.0, g_l=dphi0 - mu * dphi0, g_u=dphi0 - mu * dphi0)
    is_open, converged, trials = True, False, 0
    phi_t, dphi_t = -sums["score"], -dot6(sums["gradient"], direction)
    psi_t, dpsi_t = (phi_t - phi0) - (mu * dphi0) * a_t, dphi_t - mu * dphi0
    while not converged and trials < 10 and not (psi_t <= 0.0 and dphi_t <= -nu * dphi0):
        if is_open:
            a_t = mt_trial(s["a_l"], s["f_l"], s["g_l"], s["a_u"], s["f_u"], s["g_u"], a_t, psi_t, dpsi_t)
        else:
            a_t = mt_trial(s["a_l"], s["f_l"], s["g_l"], s["a_u"], s["f_u"], s["g_u"], a_t, phi_t, dphi_t)
        a_t = max_of(min_of(a_t, step_max), step_min)
        x = [p[r] + direction[r] * a_t for r in range(6)]
        run.evaluate(x, EVAL_GRADIENT, sums)
        phi_t, dphi_t = -sums["score"], -dot6(sums["gradient"], direction)
        psi_t, dpsi_t = (phi_t - phi0) - (mu * dphi0) * a_t, dphi_t - mu * dphi0
        if is_open and psi_t <= 0.0 and dpsi_t >= 0.0:
            is_open = False
            s["f_l"] = (s["f_l"] + phi0) - (mu * dphi0) * s["a_l"]
            s["g_l"] = s["g_l"] + mu * dphi0
            s["f_u"] = (s["f_u"] + phi0) - (mu * dphi0) * s["a_u"]
            s["g_u"] = s["g_u"] + mu * dphi0
        converged = mt_update(s, a_t, psi_t, dpsi_t) if is_open else mt_update(s, a_t, phi_t, dphi_t)
        trials += 1
    if trials > 0:
        run.evaluate(x, EVAL_HESSIAN, sums)
    return a_t


def align(cells, source, target=None, guess=None, o=None):
    """dliom_ndt_align's result as a dict, with the final points under "aligned".  target: the target's points, for the
    fitness score (None: no index, NaN and 0)."""
    o = o or options()
    p = pose_of_guess(np.eye(4) if guess is None else guess)
    run = Run(cells, source, o)
    sums = {}
    run.evaluate(p, EVAL_ALL, sums)
    res = dict(converged=0, reason=NOT_CONVERGED, iterations=0)
    it = 0
    while True:
        delta = newton_step(sums["hessian"], sums["gradient"])
        s = fsqrt(dot6(delta, delta))
        if s == 0.0 or s != s:
            res.update(converged=1 if s == s else 0, reason=ZERO_STEP, iterations=it)
            break
        direction = [div(delta[r], s) for r in range(6)]
        a = step_length(run, p, direction, s, o, sums)
        p = [p[r] + direction[r] * a for r in range(6)]
        if it > o["maximum_iterations"] or (it > 0 and abs(a) < o["transformation_epsilon"]):
            res.update(converged=1, reason=ITERATIONS if it > o["maximum_iterations"] else EPSILON, iterations=it + 1)
            break
        it += 1
    n = len(np.asarray(source).reshape(-1, 3))
    R, t, _, _ = pose_terms(p)
    with np.errstate(all="ignore"):
        aligned = ic.transform_points(R, t, source)
    res.update(p=np.array(p), transform=transform_of(p), score=sums["score"], transformation_probability=div(sums["score"], float(n)),
               pairs=sums["pairs"], evaluations_with_hessian=run.with_hessian, evaluations_without_hessian=run.without_hessian,
               aligned=aligned, fitness_score=float("nan"), fitness_count=0)
    if target is not None:
        j, d2 = ic.nn_search(aligned, target, ic.INF)
        has = j >= 0
        res["fitness_count"] = int(has.sum())
        if has.any():
            res["fitness_score"] = float(tree_sum(np.where(has, d2, 0).astype(np.float64))[0]) / res["fitness_count"]
    return res


# ---- the adapter's filter (dliom_cartographer.h registration::ApproximateVoxelGrid) ----------------------------------------
def approximate_voxel_grid(points, leaf):
    """pcl::ApproximateVoxelGrid as PCL 1.8.0 runs it, sequential: a table of 512 slots, float sums in stream order"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    inv = np.float32(1.0) / np.float32(leaf)
    slots, out = {}, []

    def flush(entry):
        count = np.float32(entry[4])
        out.append([entry[1] / count, entry[2] / count, entry[3] / count])

    for x, y, z in p:
        ix, iy, iz = int(math.floor(x * inv)), int(math.floor(y * inv)), int(math.floor(z * inv))
        h = ix * 7171 + iy * 3079 + iz * 4231
        h = ((h + 2 ** 31) % 2 ** 32 - 2 ** 31) & 511  # int arithmetic
        e = slots.get(h)
        if e is not None and e[0] != (ix, iy, iz):
            flush(e)
            e = None
        if e is None:
            e = slots[h] = [(ix, iy, iz), np.float32(0), np.float32(0), np.float32(0), 0]
        e[1], e[2], e[3], e[4] = e[1] + x, e[2] + y, e[3] + z, e[4] + 1
    for h in sorted(slots):
        flush(slots[h])
    return np.array(out, np.float32).reshape(-1, 3)
