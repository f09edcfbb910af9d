"""Synthetic world, LiDAR scans and trajectory for tests and bench.py (numpy only).

World and scan model are the ones SURVEY.md §8(d) fixes (after the generator in the reference's
local_trajectory_builder_3d_test.cc:117-250): a closed scene so that every ray returns -- a 30 m
axis-aligned cube centred at the origin plus 100 spheres of radius 0.5 m placed at
10 * normalize(U(-1,1)^3), seed 42 -- scanned by a B-beam x A-azimuth spinning LiDAR with
elevations -15..+15 degrees, direction Rz(phi) * Ry(theta) * x, per-point relative time
t = -T (1 - k/(AB-1)) (last point 0), T = 0.1 s, and the corkscrew trajectory
p = (sin 4t, 1 - cos 4t, t), rotation 0.3 t about (1,-1,2)/sqrt(6).

Second scene family (round 4, VERDICT r3: "a world with a floor"): `with scene("ground"):` switches every function of
this module to an outdoor yard -- a ground plane 1.8 m below the sensor's start height, a 120 m x 90 m walled yard
(walls 12 m high, open sky above), 40 axis-aligned boxes (cars to buildings), 90 posts and low walls near the path and 12 spheres, scanned with elevations
-25..+15 degrees and a 100 m range limit.  Rays into the sky or past the range limit do NOT return: a scan has fewer
points than beams x azimuths (ragged), the floor puts > 15 000 returns of a 64 x 1024 scan into one 0.2 m height slice,
and returns reach 60-100 m (HybridGrid bits 5 at 10 cm).  The default trajectory there is a level arc
(set_trajectory(10, 0.4, climb=0, axis=(0, 0, 1)) is applied by the context manager and undone on exit).
"""
import contextlib

import numpy as np

CUBE_HALF = 15.0
NUM_BUBBLES = 100
BUBBLE_RADIUS = 0.5


# ---------------------------------------------------------------- scene families
SCENE = {"name": "cube"}
GROUND_Z = -1.8
YARD_HALF = np.array([60.0, 45.0])
WALL_TOP = 10.2
GROUND_MAX_RANGE = 100.0
ELEVATION = {"cube": (-15.0, 15.0), "ground": (-25.0, 15.0)}


def set_scene(name):
    if name not in ELEVATION:
        raise ValueError(name)
    SCENE["name"] = name


@contextlib.contextmanager
def scene(name, trajectory=True):
    """Scene family for the duration of a `with` block (module state: tests must not leak it)."""
    keep_scene, keep_traj = SCENE["name"], dict(TRAJ)
    set_scene(name)
    if trajectory and name == "ground":
        set_trajectory(10.0, 0.4, climb=0.0, axis=(0.0, 0.0, 1.0), spin=0.3)
    try:
        yield
    finally:
        SCENE["name"] = keep_scene
        TRAJ.clear()
        TRAJ.update(keep_traj)


def bubbles(seed=42):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-1.0, 1.0, size=(NUM_BUBBLES, 3))
    if SCENE["name"] == "ground":  # a dozen spheres standing on the ground, 8-40 m out
        rng = np.random.RandomState(seed + 1)
        ang = rng.uniform(0, 2 * np.pi, 12)
        rad = rng.uniform(8.0, 40.0, 12)
        return np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(12, GROUND_Z + BUBBLE_RADIUS)], axis=1)
    return 10.0 * v / np.linalg.norm(v, axis=1, keepdims=True)


def ground_boxes(seed=43):
    """(lo, hi) corners of the yard's boxes: 40 of them, 1-8 m wide, 1.4-8 m high, standing on the ground, none within
    5 m of the origin-centred arc the sensor drives."""
    rng = np.random.RandomState(seed)
    lo, hi = [], []
    while len(lo) < 40:
        c = rng.uniform(-1.0, 1.0, 2) * (YARD_HALF - 6.0)
        size = rng.uniform(1.0, 8.0, 2)
        h = rng.uniform(1.4, 8.0)
        if np.hypot(c[0], c[1] - 10.0) < 16.0 + 0.5 * np.hypot(*size) and np.hypot(c[0], c[1] - 10.0) > 4.0 - 0.5 * np.hypot(*size):
            continue  # the arc of radius 10 around (0, 10) +- 6 m stays free
        lo.append([c[0] - 0.5 * size[0], c[1] - 0.5 * size[1], GROUND_Z])
        hi.append([c[0] + 0.5 * size[0], c[1] + 0.5 * size[1], GROUND_Z + h])
    # ... and 90 posts, bollards and low walls 2.5 - 14 m from the arc: what a street offers the matchers within the 15 - 20 m
    # of the high-resolution filters (a bare floor does not constrain x and y: the correlative matcher then picks the first
    # of many equal scores and the chain drifts by its window per scan -- the reference's behaviour, not a useful benchmark)
    while len(lo) < 130:
        ang = rng.uniform(0, 2 * np.pi)
        rad = 10.0 + rng.choice([-1.0, 1.0]) * rng.uniform(2.5, 14.0)
        if rad < 0.5:
            continue
        c = np.array([rad * np.sin(ang), 10.0 - rad * np.cos(ang)])
        if np.any(np.abs(c) > YARD_HALF - 2.0):
            continue
        size = rng.uniform(0.25, 0.7, 2) if rng.rand() < 0.7 else np.array([rng.uniform(1.5, 4.0), 0.3])[::rng.choice([1, -1])]
        h = rng.uniform(0.8, 4.0)
        lo.append([c[0] - 0.5 * size[0], c[1] - 0.5 * size[1], GROUND_Z])
        hi.append([c[0] + 0.5 * size[0], c[1] + 0.5 * size[1], GROUND_Z + h])
    return np.array(lo), np.array(hi)


def _cast_ground(o, d, centers):
    """Nearest return along each ray in the yard; np.inf where the ray leaves through the sky or exceeds the range."""
    o = np.broadcast_to(np.asarray(o, dtype=np.float64), d.shape)
    best = np.full(d.shape[0], np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = (GROUND_Z - o[:, 2]) / d[:, 2]
        best = np.where((d[:, 2] < 0) & (tg > 0), tg, best)
        # yard walls (inside faces), up to WALL_TOP
        for axis in (0, 1):
            for sign in (-1.0, 1.0):
                t = (sign * YARD_HALF[axis] - o[:, axis]) / d[:, axis]
                z = o[:, 2] + t * d[:, 2]
                other = o[:, 1 - axis] + t * d[:, 1 - axis]
                ok = (t > 1e-9) & (d[:, axis] * sign > 0) & (z <= WALL_TOP) & (z >= GROUND_Z) & (np.abs(other) <= YARD_HALF[1 - axis])
                best = np.where(ok & (t < best), t, best)
        lo, hi = ground_boxes()
        for bl, bh in zip(lo, hi):  # slab test
            t1 = (bl - o) / d
            t2 = (bh - o) / d
            tn = np.nanmax(np.minimum(t1, t2), axis=1)
            tf = np.nanmin(np.maximum(t1, t2), axis=1)
            ok = (tn <= tf) & (tn > 1e-9)
            best = np.where(ok & (tn < best), tn, best)
    for c in centers:
        oc = o - c
        bq = (d * oc).sum(axis=1)
        cq = (oc * oc).sum(axis=1) - BUBBLE_RADIUS ** 2
        disc = bq * bq - cq
        hit = disc > 0
        t = np.where(hit, -bq - np.sqrt(np.where(hit, disc, 0.0)), np.inf)
        t = np.where(t > 1e-9, t, np.inf)
        best = np.minimum(best, t)
    return np.where(best <= GROUND_MAX_RANGE, best, np.inf)


def quat_from_axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    s = np.sin(0.5 * angle)
    return np.array([np.cos(0.5 * angle), axis[0] * s, axis[1] * s, axis[2] * s])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def quat_to_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_compose(a, b):
    """[t,q] (x) [t,q] in double (plain formulas; test scaffolding, not a parity path)."""
    Ra = quat_to_matrix(a[3:])
    t = Ra @ b[:3] + a[:3]
    q = quat_mul(a[3:], b[3:])
    q = q / np.linalg.norm(q)
    return np.concatenate([t, q])


def pose_inverse(a):
    q = np.array([a[3], -a[4], -a[5], -a[6]])
    t = -(quat_to_matrix(q) @ a[:3])
    return np.concatenate([t, q])


# p(t) = (R sin wt, R (1 - cos wt), t).  The reference test's corkscrew is R = 1 m, w = 4 rad/s (4 m/s on a 1 m
# circle: 16 m/s^2); set_trajectory(10.0, 0.4) is a vehicle-like arc (4 m/s, 1.6 m/s^2) for the streaming tool.
TRAJ = {"radius": 1.0, "omega": 4.0, "climb": 1.0, "axis": (1.0, -1.0, 2.0), "spin": 0.3}


def set_trajectory(radius=1.0, omega=4.0, climb=1.0, axis=(1.0, -1.0, 2.0), spin=0.3):
    TRAJ["radius"], TRAJ["omega"], TRAJ["climb"] = float(radius), float(omega), float(climb)
    TRAJ["axis"], TRAJ["spin"] = tuple(float(a) for a in axis), float(spin)


def _axis():
    a = np.asarray(TRAJ["axis"], dtype=np.float64)
    return a / np.linalg.norm(a)


def trajectory_pose(t):
    """Corkscrew pose at time t (seconds)."""
    R, w = TRAJ["radius"], TRAJ["omega"]
    p = np.array([R * np.sin(w * t), R * (1.0 - np.cos(w * t)), TRAJ["climb"] * t])
    q = quat_from_axis_angle(TRAJ["axis"], TRAJ["spin"] * t)
    return np.concatenate([p, q])


def beam_directions(num_beams, num_azimuths):
    """Unit directions in the sensor frame, azimuth-major (a * B + b), plus relative times."""
    b = np.arange(num_beams)
    e_lo, e_hi = ELEVATION[SCENE["name"]]
    # "elevation" e: the reference's generator looks DOWN for positive theta (Ry(theta) x), kept for the cube; the yard's
    # -25..+15 degrees are true elevations (25 down, 15 up), i.e. theta = -e
    if SCENE["name"] == "cube":
        theta = np.deg2rad(e_lo + (e_hi - e_lo) * b / max(num_beams - 1, 1))
    else:
        theta = -np.deg2rad(e_lo + (e_hi - e_lo) * b / max(num_beams - 1, 1))
    a = np.arange(num_azimuths)
    phi = 2.0 * np.pi * a / num_azimuths
    # Rz(phi) * Ry(theta) * x_hat ; Ry(theta) x = (cos th, 0, -sin th): positive theta looks down
    ct, st = np.cos(theta), np.sin(theta)
    cp, sp = np.cos(phi), np.sin(phi)
    d = np.stack([np.outer(cp, ct), np.outer(sp, ct), np.tile(-st, (num_azimuths, 1))], axis=-1)
    d = d.reshape(-1, 3)
    k = np.arange(num_beams * num_azimuths)
    rel_t = -0.1 * (1.0 - k / max(num_beams * num_azimuths - 1, 1))
    return d, rel_t


def cast(origin, dirs, centers=None):
    """Range along each ray from `origin` (inside the cube) to the nearest surface."""
    if centers is None:
        centers = bubbles()
    o = np.asarray(origin, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    if SCENE["name"] == "ground":
        return _cast_ground(o, d, centers)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_pos = (CUBE_HALF - o) / d
        t_neg = (-CUBE_HALF - o) / d
    t_box = np.where(d > 0, t_pos, np.where(d < 0, t_neg, np.inf)).min(axis=1)
    best = t_box
    for c in centers:
        oc = o - c
        bq = d @ oc
        cq = oc @ oc - BUBBLE_RADIUS ** 2
        disc = bq * bq - cq
        hit = disc > 0
        t = np.where(hit, -bq - np.sqrt(np.where(hit, disc, 0.0)), np.inf)
        t = np.where(t > 1e-9, t, np.inf)
        best = np.minimum(best, t)
    return best


def scan(pose, num_beams=64, num_azimuths=1024, noise_sigma=0.0, noise_seed=7, centers=None):
    """One scan taken at `pose` ([t,q] world<-sensor).  Returns float32 points in the SENSOR frame
    (n,3) and the per-point relative times."""
    dirs_s, rel_t = beam_directions(num_beams, num_azimuths)
    R = quat_to_matrix(pose[3:])
    dirs_w = dirs_s @ R.T
    rng_ = cast(pose[:3], dirs_w, centers)
    if noise_sigma > 0:
        rng_ = rng_ + np.random.RandomState(noise_seed).normal(0.0, noise_sigma, size=rng_.shape)
    back = np.isfinite(rng_)  # the yard has rays that do not return; the cube returns every ray
    pts = (dirs_s[back] * rng_[back, None]).astype(np.float32)
    return pts, rel_t[back].astype(np.float32)


def transform_points(pose, pts):
    """float64 transform of points by [t,q] (scaffolding for building submaps)."""
    R = quat_to_matrix(pose[3:])
    return (np.asarray(pts, dtype=np.float64) @ R.T + pose[:3]).astype(np.float32)


def perturb_pose(pose, max_translation, max_angle_deg, seed=13):
    rng = np.random.RandomState(seed)
    dt = rng.uniform(-max_translation, max_translation, size=3)
    axis = rng.uniform(-1, 1, size=3)
    ang = np.deg2rad(rng.uniform(-max_angle_deg, max_angle_deg))
    return pose_compose(pose, np.concatenate([dt, quat_from_axis_angle(axis, ang)]))


def range_filter(pts, max_range):
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    return pts[r <= max_range]


# ---------------------------------------------------------------- motion-distorted scans + IMU (config 3)
AXIS = np.array([1.0, -1.0, 2.0]) / np.sqrt(6.0)  # the default trajectory's; _axis() is the current one
GRAVITY = np.array([0.0, 0.0, 9.80511])  # trajectory_builder_3d.lua:92; the IMU measures R^T (a + G)


def trajectory_velocity(t):
    R, w = TRAJ["radius"], TRAJ["omega"]
    return np.array([R * w * np.cos(w * t), R * w * np.sin(w * t), TRAJ["climb"]])


def trajectory_state(t):
    """[P(3), Q(4), V(3), Ba(3), Bg(3)] of the corkscrew at time t."""
    pose = trajectory_pose(t)
    return np.concatenate([pose, trajectory_velocity(t), np.zeros(6)])


def imu_samples(t0, t1, rate=200.0, noise=None, seed=11):
    """Specific force R^T (a + G) and body rate at t0, t0 + 1/rate, ..., t1 (inclusive)."""
    n = int(round((t1 - t0) * rate)) + 1
    ts = t0 + np.arange(n) / rate
    R, w = TRAJ["radius"], TRAJ["omega"]
    acc_w = np.stack([-R * w * w * np.sin(w * ts), R * w * w * np.cos(w * ts), np.zeros(n)], axis=1) + GRAVITY
    acc = np.stack([quat_to_matrix(quat_from_axis_angle(_axis(), TRAJ["spin"] * t)).T @ a for t, a in zip(ts, acc_w)])
    gyr = np.tile(TRAJ["spin"] * _axis(), (n, 1))  # rotation about a fixed axis: body rate == world rate
    if noise is not None:
        rng = np.random.RandomState(seed)
        acc = acc + noise[0] * rng.normal(size=acc.shape)
        gyr = gyr + noise[1] * rng.normal(size=gyr.shape)
    return 1.0 / rate, acc, gyr


def cast_many(origins, dirs, centers=None):
    """cast() with one origin per ray."""
    if centers is None:
        centers = bubbles()
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    if SCENE["name"] == "ground":
        return _cast_ground(o, d, centers)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_pos = (CUBE_HALF - o) / d
        t_neg = (-CUBE_HALF - o) / d
    best = np.where(d > 0, t_pos, np.where(d < 0, t_neg, np.inf)).min(axis=1)
    for c in centers:
        oc = o - c
        bq = (d * oc).sum(axis=1)
        cq = (oc * oc).sum(axis=1) - BUBBLE_RADIUS ** 2
        disc = bq * bq - cq
        hit = disc > 0
        t = np.where(hit, -bq - np.sqrt(np.where(hit, disc, 0.0)), np.inf)
        t = np.where(t > 1e-9, t, np.inf)
        best = np.minimum(best, t)
    return best


def moving_scan(t_end, num_beams=64, num_azimuths=1024, centers=None):
    """A scan swept while the sensor flies the corkscrew: point k is measured at t_end + rel_t[k] in the
    sensor frame OF THAT INSTANT.  Returns float32 [x, y, z, rel_t] rows."""
    dirs_s, rel_t = beam_directions(num_beams, num_azimuths)
    ts = t_end + rel_t
    R, w = TRAJ["radius"], TRAJ["omega"]
    pos = np.stack([R * np.sin(w * ts), R * (1.0 - np.cos(w * ts)), TRAJ["climb"] * ts], axis=1)
    ang = TRAJ["spin"] * ts
    ax = _axis()
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    # Rodrigues: R d = d + sin(a) K d + (1 - cos a) K K d
    Kd = dirs_s @ K.T
    KKd = Kd @ K.T
    dirs_w = dirs_s + np.sin(ang)[:, None] * Kd + (1.0 - np.cos(ang))[:, None] * KKd
    rng_ = cast_many(pos, dirs_w, centers)
    back = np.isfinite(rng_)
    return np.concatenate([dirs_s[back] * rng_[back, None], rel_t[back, None]], axis=1).astype(np.float32)


# ---- pose graphs (OptimizationProblem3D::Solve) ------------------------------------------------------------------------
def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def _quat_rotate(q, v):
    qv = np.array([0.0, v[0], v[1], v[2]])
    return _quat_mul(_quat_mul(q, qv), q * np.array([1.0, -1.0, -1.0, -1.0]))[1:]


def _quat_of(rotation_vector):
    angle = np.linalg.norm(rotation_vector)
    if angle < 1e-12:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * np.asarray(rotation_vector) / angle])


def pose7_compose(a, b):
    """a * b of poses [t, q wxyz]."""
    q = _quat_mul(a[3:], b[3:])
    return np.concatenate([_quat_rotate(a[3:], b[:3]) + a[:3], q / np.linalg.norm(q)])


def pose7_inverse(a):
    q = a[3:] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([-_quat_rotate(q, a[:3]), q])


def pose_graph(num_submaps, num_nodes, loop_groups=0, seed=0, every_nodes_to_find_constraint=3, drift=(0.02, 0.002),
               noise=(0.01, 0.002), frozen_submaps=0):
    """A pose graph as PoseGraph3D hands it to OptimizationProblem3D::Solve: `num_nodes` nodes on a closed, climbing loop;
    submap a starts at node a * num_nodes // (num_submaps - 1), and every node is constrained (INTRA_SUBMAP, weights
    matcher_*_weight of pose_graph.lua) to the two consecutive submaps it was inserted into; `loop_groups` groups of
    67 // every_nodes_to_find_constraint INTER_SUBMAP constraints (weights loop_closure_*_weight of basic_config_3d.lua)
    tie nodes of the last quarter to a submap of the first.  The initial poses carry a random-walk drift
    (metres, radians a node); the first `frozen_submaps` submaps and their nodes are constant (a frozen trajectory).
    -> dict(submaps (S, 7), nodes (N, 7), constraints (structured: submap, node, zbar, translation_weight,
    rotation_weight), submap_constant, node_constant, truth_nodes)."""
    rng = np.random.RandomState(seed)
    segments = max(num_submaps - 1, 1)
    truth = np.zeros((num_nodes, 7))
    for j in range(num_nodes):
        a = 2 * np.pi * j / num_nodes
        truth[j, :3] = [20 * np.cos(a), 20 * np.sin(a), 0.5 * np.sin(2 * a)]
        truth[j, 3:] = _quat_mul(_quat_of([0, 0, a + np.pi / 2]), _quat_of([0.05 * np.sin(3 * a), 0.04 * np.cos(2 * a), 0]))
    start = [min(a * num_nodes // segments, num_nodes - 1) for a in range(num_submaps)]
    truth_submaps = truth[start].copy()
    # the drifting estimate: a random walk of small relative errors along the trajectory
    nodes = np.zeros_like(truth)
    error = np.array([0, 0, 0, 1.0, 0, 0, 0])
    for j in range(num_nodes):
        step = np.concatenate([rng.normal(0, drift[0], 3), _quat_of(rng.normal(0, drift[1], 3))])
        error = pose7_compose(error, step)
        nodes[j] = pose7_compose(error, truth[j])
    submaps = nodes[start].copy()
    rows = []

    def constrain(a, j, tw, rw):
        z = pose7_compose(pose7_inverse(truth_submaps[a]), truth[j])
        z = pose7_compose(z, np.concatenate([rng.normal(0, noise[0], 3), _quat_of(rng.normal(0, noise[1], 3))]))
        rows.append((a, j, z, tw, rw))
    for j in range(num_nodes):
        a = min(j * segments // num_nodes, num_submaps - 1)
        constrain(a, j, 5e2, 1.6e3)
        if a + 1 < num_submaps and num_submaps > 1:
            constrain(a + 1, j, 5e2, 1.6e3)
    per_group = 67 // every_nodes_to_find_constraint
    for k in range(loop_groups):
        a = int(rng.randint(0, max(num_submaps // 4, 1)))
        first = int(rng.randint(3 * num_nodes // 4, max(num_nodes - per_group * every_nodes_to_find_constraint, 3 * num_nodes // 4 + 1)))
        for i in range(per_group):
            j = first + i * every_nodes_to_find_constraint
            if j < num_nodes:
                constrain(a, j, 1e4, 1e2)
    constraints = np.zeros(len(rows), dtype=[("submap", "<i4"), ("node", "<i4"), ("zbar", "<f8", 7), ("translation_weight", "<f8"),
                                             ("rotation_weight", "<f8")])
    for i, (a, j, z, tw, rw) in enumerate(rows):
        constraints[i] = (a, j, z, tw, rw)
    submap_constant = (np.arange(num_submaps) < frozen_submaps).astype(np.uint8)
    node_constant = np.array([min(j * segments // num_nodes, num_submaps - 1) < frozen_submaps for j in range(num_nodes)], dtype=np.uint8)
    return dict(submaps=submaps, nodes=nodes, constraints=constraints, submap_constant=submap_constant, node_constant=node_constant,
                truth_nodes=truth)
