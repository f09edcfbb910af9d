"""Scenes for the IMU-LiDAR initialisation's tests: frames (a pose in the first laser frame and the preintegration that ran
up to it) from tests/imu_motion.py's analytic motion, with noise-free 200 Hz IMU through dliom_imu_integrator and exact
relative poses."""
import numpy as np
from scipy.spatial.transform import Rotation

import imu_motion

G = 9.80511
TRANSFORM_LB = np.array([0.05, -0.02, 0.10, 1.0, 0.0, 0.0, 0.0])
NOISE = (0.01, 0.001, 0.0001, 0.00001)


def frames_of(dl, num_frames=8, seed=5, at_rest=False, frame0_preintegration=True, spacing=0.1, start=1.0, max_frequency=0.7):
    """-> (frames [(pose7, preintegration or None)], truth dict(gravity_in_laser, local_velocities)).  The laser's world
    pose is (p + R tlb, R) for the IMU's (p, R): what the initializer's equations take T_i to be."""
    m = imu_motion.RandomMotion(seed, gravity=G, translation_amplitude=0.0 if at_rest else 1.0,
                                rotation_amplitude=0.0 if at_rest else 0.4, max_frequency=max_frequency)
    times = start + spacing * np.arange(num_frames)
    tlb = TRANSFORM_LB[:3]
    R0 = m.rotation(times[0])
    T0 = m.position(times[0]) + R0 @ tlb
    integrator = dl.ImuIntegrator(np.zeros(3), np.zeros(3), NOISE)
    frames = []
    for k, t in enumerate(times):
        R = m.rotation(t)
        q = Rotation.from_matrix(R0.T @ R).as_quat()  # x, y, z, w
        pose = np.concatenate([R0.T @ (m.position(t) + R @ tlb - T0), [q[3], q[0], q[1], q[2]]])
        pre = None
        if k > 0 or frame0_preintegration:
            integrator.reset(np.zeros(3), np.zeros(3))
            steps = int(round(spacing * 200.0))
            dt = spacing / steps
            for j in range(steps + 1):  # the first sample only opens the mid-point rule: it integrates nothing
                at = t - spacing + j * dt
                integrator.push_back(dt, m.specific_force(at), m.body_rate(at))
            pre = integrator.get()
        frames.append((pose, pre))
    integrator.close()
    truth = {"gravity_in_laser": R0.T @ m.G, "local_velocities": np.array([m.rotation(t).T @ m.velocity(t) for t in times])}
    return frames, truth
