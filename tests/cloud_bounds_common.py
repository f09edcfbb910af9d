"""Shared by tests/test_cloud_bounds_host.py (CPU) and tests/test_gpu_cloud_bounds.py (device): the reference of the bound
a cloud carries (dliom_cloud_bounds: max_i |p_i|), and PRESCRIBED inputs for every stage that makes a cloud on the device.
Nothing here is random in what it tests: the sizes sit around the wavefront (64) and workgroup (256) shapes, and the
farthest point -- kept, or removed by the stage -- is put at the indices where a reduction loses a value: the first and
last lane of a wavefront, the first and last thread of a workgroup, the last point, a last workgroup of one point, the
only kept point of a wavefront.  (Directions and the radii of the other points come from a fixed seed.)"""
import collections

import numpy as np

f32 = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, 65537]
POSITIONS = [0, 63, 64, 255, 256]
EDGE = 0.5  # the voxel edge of the lattice clouds (voxel filters, outlier remover)
RANGE_MIN, RANGE_MAX = 1.0, 20.0
ADAPTIVE_ALL, ADAPTIVE_CROPPED = (EDGE, 1.0, 100.0), (EDGE, 1.0, 45.0)  # (max_length, min_num_points, max_range)
CHUNK = 64  # points_batch.hip kChunk: pulses a sampler thread replays

Case = collections.namedtuple("Case", "name points keep params")  # keep: bool[n], what the stage must keep


def ref_max_norm(points):
    """cloud_max_norm (core.hip) in numpy float32: s = x*x + (y*y + z*z); best starts at 0 and takes s only where
    s > best (a NaN never wins, +inf does); sqrt(best)."""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        s = x * x + (y * y + z * z)
        assert s.dtype == f32
        s = s[s > f32(0)]  # drops NaN, and zeros, which cannot raise a maximum that starts at 0
        best = s.max() if len(s) else f32(0)
        return f32(np.sqrt(f32(best)))


def ref_max_norm_loop(points):
    """The same as a plain loop (the host test ties the two together)."""
    best = f32(0)
    with np.errstate(all="ignore"):
        for x, y, z in np.asarray(points, dtype=f32).reshape(-1, 3):
            s = f32(f32(x * x) + f32(f32(y * y) + f32(z * z)))
            if s > best:
                best = s
        return f32(np.sqrt(best))


def bits(v):
    return np.asarray(v, dtype=f32).tobytes()


def positions(n):
    return sorted({p for p in POSITIONS + [n - 1] if 0 <= p < n})


def masks(n, first_kept=False):
    """-> [(name, keep, far_kept or None, far_removed or None)].  first_kept: the stage always keeps point 0 and can only
    remove a point that follows a kept one (the voxel filters); the cases it cannot have are left out."""
    base = (np.arange(n) % 3) != 1
    out = []

    def done(name, keep, far_kept, far_removed):
        if first_kept:
            keep[0] = True
        out.append((name, keep, far_kept, far_removed))

    for pos in positions(n):
        keep = base.copy()
        keep[pos] = True
        done("kept_far_at_%d" % pos, keep, pos, None)
        if not (first_kept and 0 < pos < 64):
            keep = base.copy()
            keep[pos // 64 * 64:pos // 64 * 64 + 64] = False
            keep[pos] = True
            done("only_kept_of_its_wavefront_at_%d" % pos, keep, pos, None)
        if not (first_kept and pos == 0):
            keep = base.copy()
            keep[pos] = False
            other = pos - 1 if pos > 0 else (1 if n > 1 else None)
            if other is not None:
                keep[other] = True
            done("removed_far_at_%d" % pos, keep, other, pos)
    return out


def shell(n, keep, far_kept, far_removed, radii=(2.0, 10.0, 15.0, 30.0, 40.0)):
    """Points in fixed directions: the kept ones at lo..hi metres, the farthest kept one at radii[2], the removed ones at
    radii[3] and the farthest removed one at radii[4]."""
    lo, hi, r_far_kept, r_removed, r_far_removed = radii
    rng = np.random.RandomState(1000 + n)
    d = rng.normal(size=(n, 3)) + 1e-3
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.where(keep, rng.uniform(lo, hi, n), r_removed)
    if far_kept is not None:
        r[far_kept] = r_far_kept
    if far_removed is not None:
        r[far_removed] = r_far_removed
    return np.ascontiguousarray((d * r[:, None]).astype(f32))


def lattice(n, keep, far_kept, far_removed, duplicates):
    """One point a voxel of EDGE on a 64 x 64 x k lattice about the origin (norms below 24 m), the farthest kept one in
    the voxel at x = 50 m.  duplicates (voxel filters): a removed point lies in the voxel of point 0, the farthest removed
    one in the voxel of the farthest kept one, behind it and farther out.  Else (outlier remover): a removed point has a
    voxel of its own, which gets no hit; the farthest one at x = 60 m."""
    rng = np.random.RandomState(2000 + n)
    i = np.arange(n)
    cells = np.stack([i % 64 - 32, (i // 64) % 64 - 32, i // 4096 - 8], axis=1).astype(np.float64)
    pts = cells * EDGE + rng.uniform(-0.1, 0.1, (n, 3))
    if far_kept is not None:
        pts[far_kept] = (49.9 if duplicates and far_removed is not None else 50.0, 0.02, -0.03)
    if duplicates:
        removed = np.flatnonzero(~keep)
        pts[removed] = pts[0] + rng.uniform(-0.05, 0.05, (len(removed), 3))
    if far_removed is not None:
        pts[far_removed] = (50.2, 0.01, 0.04) if duplicates else (60.0, 0.01, 0.04)
    return np.ascontiguousarray(pts.astype(f32))


def _special_clouds(kind, n=257):
    """The value edges, as (name, points, keep, range-filter bounds): a tie, the origin (-0.0 among it), nothing kept, a
    denormal squared norm, and for the stages that pass them on a kept +inf and a kept NaN."""
    base = (np.arange(n) % 3) != 1
    voxel = kind == "voxel"
    if voxel:
        base[0] = True
    make = (lambda k, a, b: lattice(n, k, a, b, voxel)) if kind != "range" else (lambda k, a, b: shell(n, k, a, b))
    bounds = (RANGE_MIN, RANGE_MAX)
    out = []
    # two kept points tie for the maximum: p and -p have the same squared norm
    keep = base.copy()
    keep[[64, 200]] = True
    pts = make(keep, 64, None)
    pts[200] = -pts[64]
    out.append(("tie", pts, keep, bounds))
    # every kept point at the origin, one of them -0.0: the bound is +0
    keep = base.copy()
    pts = make(keep, None, None)
    pts[keep] = 0.0
    pts[np.flatnonzero(keep)[0]] = (-0.0, 0.0, -0.0)
    if voxel:  # one voxel: its first point stays
        keep = np.zeros(n, bool)
        keep[0] = True
        pts[:] = 0.0
        pts[0] = (-0.0, 0.0, -0.0)
    out.append(("origin", pts, keep, (0.0, RANGE_MAX)))
    # the squared norm of the maximum is a denormal float
    keep = base.copy()
    pts = make(keep, None, None)
    tiny = np.random.RandomState(5).uniform(-1.0, 1.0, (n, 3)) * 1e-20
    tiny[np.flatnonzero(keep)[-1]] = (1.5e-20, -1.2e-20, 0.7e-20)
    if voxel:
        keep = np.zeros(n, bool)
        keep[0] = True
        pts = tiny.copy()
        pts[0] = (1.5e-20, -1.2e-20, 0.7e-20)
    else:
        pts[keep] = tiny[keep]
    out.append(("denormal", pts.astype(f32), keep, (0.0, RANGE_MAX)))
    # nothing is kept
    keep = np.zeros(n, bool)
    out.append(("nothing_kept", np.zeros((0, 3), f32) if voxel else make(keep, None, 100), keep[:0] if voxel else keep, bounds))
    if kind == "range":  # range <= max_range holds for an infinite range when max_range is infinite; a NaN range is never kept
        keep = base.copy()
        keep[255] = True
        pts = make(keep, 64, None)
        pts[255] = (np.inf, 1.0, -2.0)
        pts[~keep] = 0.25  # the removed points: nearer than min_range
        out.append(("kept_inf", pts, keep, (RANGE_MIN, np.inf)))
    return [(name, np.ascontiguousarray(p, dtype=f32), k, b) for name, p, k, b in out]


def cases(kind, n):
    """The prescribed clouds of `kind` ("range", "remover", "voxel") at n points, the value edges with n = 257."""
    out = []
    for name, keep, far_kept, far_removed in masks(n, first_kept=kind == "voxel"):
        pts = shell(n, keep, far_kept, far_removed) if kind == "range" else lattice(n, keep, far_kept, far_removed, kind == "voxel")
        out.append(Case("%s_%d_%s" % (kind, n, name), pts, keep, (RANGE_MIN, RANGE_MAX)))
    if n == 257:
        out += [Case("%s_%s" % (kind, name), p, k, b) for name, p, k, b in _special_clouds(kind)]
    return out


def range_keep(points, bounds, origin=(0.0, 0.0, 0.0)):
    """MinMaxRangeFiteringPointsProcessor in numpy: float range, double bounds."""
    d = np.asarray(points, f32) - np.asarray(origin, f32)
    with np.errstate(all="ignore"):
        r = np.sqrt((d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])).astype(f32)).astype(f32).astype(np.float64)
        return (bounds[0] <= r) & (r <= bounds[1])


def premise(case):
    """What a case claims about itself.  -> (bound of the survivors, bound of the input)"""
    kept, everything = ref_max_norm(case.points[case.keep]), ref_max_norm(case.points)
    if "removed_far" in case.name:
        assert everything > kept, (case.name, everything, kept)
    if "kept_far" in case.name or "only_kept" in case.name:
        assert kept > 0
    return kept, everything


# ---- the sampler ------------------------------------------------------------------------------------------------------
def sampler_keep(ratio, n, pulses=0, samples=0):
    """common::FixedRatioSampler::Pulse, n times."""
    keep = np.zeros(n, bool)
    for i in range(n):
        pulses += 1
        if float(samples) / float(pulses) < ratio:
            keep[i] = True
            samples += 1
    return keep


def sampler_first_pass_keep(ratio, n):
    """What the device's FIRST pass flags from state (0, 0) (sampler_chunks_kernel): chunk c > 0 starts from the guess
    clamp(ceil(ratio * 64 c), 0, 64 c).  Where the guess is wrong these flags differ from sampler_keep's."""
    keep = np.zeros(n, bool)
    for c in range((n + CHUNK - 1) // CHUNK):
        first = c * CHUNK
        samples = 0 if c == 0 else int(min(max(np.ceil(np.float64(ratio) * np.float64(first)), 0.0), float(first)))
        pulses = first
        for i in range(first, min(n, first + CHUNK)):
            pulses += 1
            if float(samples) / float(pulses) < ratio:
                keep[i] = True
                samples += 1
    return keep


def sampler_cases():
    """-> [Case]; params = ratio.  The sampler decides what is kept: at each prescribed index the farthest point is a
    kept one or a removed one, as the index falls."""
    out = []
    for n in SIZES:
        keep = sampler_keep(0.5, n)
        for pos in positions(n):
            if keep[pos]:
                out.append(Case("sampler_0.5_%d_kept_far_at_%d" % (n, pos), shell(n, keep, pos, None), keep, 0.5))
            else:
                other = pos - 1 if pos > 0 and keep[pos - 1] else int(np.flatnonzero(keep)[0])
                out.append(Case("sampler_0.5_%d_removed_far_at_%d" % (n, pos), shell(n, keep, other, pos), keep, 0.5))
    n = 4097
    keep, first = sampler_keep(0.55, n), sampler_first_pass_keep(0.55, n)
    # Where the guess is wrong here (pulses 1600, 2880, 3200, 3520) it is one too HIGH: the first pass drops a pulse the
    # sequential loop keeps, and keeps none that the loop drops (test_cloud_bounds_host.py asserts both).  So the farthest
    # point is such a pulse: a bound taken before the repair passes misses it.  What this case cannot see: max_sq left
    # un-zeroed between repair passes -- that needs a pulse the first pass keeps and the loop drops, farther out than every
    # kept one, and no ratio and start state tried has one.
    missed = np.flatnonzero(~first & keep)
    assert len(missed) > 0, "0.55 over 4097 pulses has chunks whose guessed start is wrong"
    out.append(Case("sampler_0.55_repaired_kept_far_at_%d" % missed[0], shell(n, keep, int(missed[0]), None), keep, 0.55))
    out.append(Case("sampler_0_nothing_kept", shell(257, np.zeros(257, bool), None, 100), np.zeros(257, bool), 0.0))
    keep = sampler_keep(0.5, 257)
    kept = np.flatnonzero(keep)
    pts = shell(257, keep, int(kept[40]), None)
    pts[kept[100]] = (1.0, np.inf, -2.0)
    out.append(Case("sampler_kept_inf", pts, keep, 0.5))
    pts = shell(257, keep, int(kept[40]), None)
    pts[kept[100]] = (np.nan, 1.0, 2.0)
    pts[kept[3]] = (1e30, np.nan, 0.0)
    pts[kept[-1]] = (np.nan, np.nan, np.nan)
    out.append(Case("sampler_kept_nan", pts, keep, 0.5))
    pts = shell(257, keep, None, None)
    pts[keep] = 0.0
    pts[kept[5]] = (0.0, -0.0, 0.0)
    out.append(Case("sampler_origin", pts, keep, 0.5))
    pts = shell(257, keep, int(kept[40]), None)
    pts[kept[90]] = -pts[kept[40]]
    out.append(Case("sampler_tie", pts, keep, 0.5))
    pts = shell(257, keep, None, None)
    pts[keep] = (np.random.RandomState(6).uniform(-1.0, 1.0, (len(kept), 3)) * 1e-20).astype(f32)
    pts[kept[-1]] = (1.5e-20, -1.2e-20, 0.7e-20)
    out.append(Case("sampler_denormal", pts, keep, 0.5))
    return out


# ---- the front end's returns cloud (dliom_add_range_data) ---------------------------------------------------------------
FRONTEND_VFS, FRONTEND_PERIOD = 0.15, 0.1  # voxel edges 0.075 (timed ranges) and 0.15 (returns); 4095 edges: 307 m, 614 m
FRONTEND_RANGES = (0.0, 55.0)
FRONTEND_FAR = (1.0, 1000.0)  # the gate of the cases with a range beyond 4095 voxel edges


def frontend_poses():
    from dliom import synth
    return synth.trajectory_pose(0.4), synth.trajectory_pose(0.5)


def _frontend_xyzt(points):
    n = len(points)
    rel_t = -FRONTEND_PERIOD * (1.0 - np.arange(n) / max(n - 1, 1))  # the last range at the scan's stamp
    return np.ascontiguousarray(np.concatenate([points, rel_t[:, None]], axis=1), dtype=f32)


def frontend_cases(n):
    """-> [Case] whose points are timed ranges xyzt (n, 4) in the sensor frame, params = (min_range, max_range).  The kept
    ranges lie one a voxel on the lattice (0.5 m apart, at least 0.3 m on some axis: no voxel of 0.15 m holds two, however
    the de-skew turns them), so the returns cloud is the keep mask's compaction and the farthest return sits where the case
    puts it.  A range is removed by the gate (70 m and 80 m out, max_range 55 m), or ("voxel_removed") by the first
    filter, as the later point of the farthest kept range's voxel, 2 cm farther out.  With n = 257 also: a range beyond
    4095 edges of both filters, kept, so that both stages leave their packed path; nothing kept.  (The cloud is a
    transform's output: a tie, the origin or a denormal among the inputs does not come out as one; a NaN range fails the
    gate and an infinite one comes out of the rotation as NaN, so neither is a case here.)"""
    out = []
    for name, keep, far_kept, far_removed in masks(n):
        pts = lattice(n, keep, far_kept, far_removed, False)
        rng = np.random.RandomState(3000 + n)
        d = rng.normal(size=(n, 3)) + 1e-3
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts[~keep] = (d * 70.0).astype(f32)[~keep]
        if far_removed is not None:
            pts[far_removed] = (d[far_removed] * 80.0).astype(f32)
        out.append(Case("frontend_%d_%s" % (n, name), _frontend_xyzt(pts), keep, FRONTEND_RANGES))
        if far_removed is not None and far_kept is not None and far_kept < far_removed:
            pts = pts.copy()
            pts[far_removed] = pts[far_kept] + f32([0.02, 0.0, 0.0])
            out.append(Case("frontend_%d_voxel_%s" % (n, name), _frontend_xyzt(pts), keep, FRONTEND_RANGES))
    if n == 257:
        keep = np.ones(n, bool)
        pts = lattice(n, keep, None, None, False)
        pts[64] = (700.0, 3.0, -2.0)
        out.append(Case("frontend_general_path_kept_far_at_64", _frontend_xyzt(pts), keep, FRONTEND_FAR))
        keep = keep.copy()
        keep[200] = False
        pts = pts.copy()
        pts[200] = (-1100.0, 1.0, 4.0)
        out.append(Case("frontend_general_path_removed_far_at_200", _frontend_xyzt(pts), keep, FRONTEND_FAR))
        none = np.zeros(n, bool)
        pts = lattice(n, none, None, None, False)
        pts[:] = pts + f32([100.0, 0.0, 0.0])
        out.append(Case("frontend_nothing_kept", _frontend_xyzt(pts), none, FRONTEND_RANGES))
    return out


def frontend_oracle(orc, case, points=None):
    """The oracle's AddRangeData restatement on a case -> (returns in the tracking frame, input indices of the returns)."""
    prev, cur = frontend_poses()
    xyzt = case.points if points is None else points
    ref = orc.deskew_and_filter(FRONTEND_PERIOD, case.params[0], case.params[1], FRONTEND_VFS, prev, cur, xyzt)
    hits = orc.voxel_filter(0.5 * f32(FRONTEND_VFS), xyzt[:, :3])
    return ref["returns_in_tracking"].astype(f32), np.asarray(hits)[ref["kind"] == 1]


# ---- the assembler ----------------------------------------------------------------------------------------------------
ASSEMBLE_RADII = (2.0, 10.0, 80.0, 120.0, 200.0)  # sensor frame; the corkscrew moves the points by a few metres


def assemble_trajectory():
    import assemble_common as ac
    times, poses = ac.corkscrew(37, ac.SPANS[37])
    return times, poses, int(times[-1])


def assemble_xyzt(points, keep):
    """Sensor-frame points with relative times: a kept point's time lies inside the trajectory, a removed one's 0.5 s
    before its first node."""
    n = len(points)
    inside = -np.linspace(0.001, 0.17, max(n, 1))[:n]
    return np.ascontiguousarray(np.concatenate([points, np.where(keep, inside, inside - 0.5)[:, None]], axis=1), dtype=f32)


def assemble_cases():
    """-> [Case] whose points are xyzt (n, 4).  Non-finite coordinates are passed through by the assembler."""
    out = []
    for n in SIZES:
        for name, keep, far_kept, far_removed in masks(n):
            out.append(Case("assemble_%d_%s" % (n, name), assemble_xyzt(shell(n, keep, far_kept, far_removed, ASSEMBLE_RADII), keep),
                            keep, None))
    n = 257
    base = (np.arange(n) % 3) != 1
    kept = np.flatnonzero(base)
    pts = shell(n, base, int(kept[40]), None, ASSEMBLE_RADII)
    pts[kept[100]] = (np.inf, 1.0, -2.0)
    out.append(Case("assemble_kept_inf", assemble_xyzt(pts, base), base, None))
    pts = shell(n, base, int(kept[40]), None, ASSEMBLE_RADII)
    pts[kept[100]] = (np.nan, 1.0, 2.0)
    pts[kept[-1]] = (np.nan, np.nan, np.nan)
    out.append(Case("assemble_kept_nan", assemble_xyzt(pts, base), base, None))
    none = np.zeros(n, bool)
    out.append(Case("assemble_nothing_kept", assemble_xyzt(shell(n, none, None, 100, ASSEMBLE_RADII), none), none, None))
    return out
