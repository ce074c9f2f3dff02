"""Robots and plans away from the infinity course, for the preprocessing and the tick
(tests/test_host_logic.py on the CPU, tests/test_gpu_general.py on the GPU): straight and circular
plans that take the branches of findBestPath's heading rule (driving_state.cpp:214-235) which the
lemniscate and random smooth arcs never take on purpose.

A plain module: the test modules import it; it is no conftest and holds no fixture.
"""
from __future__ import annotations

import numpy as np

# the plan lengths: int(0.3 M) <= 1 for M = 4, 5, 6 (no waypoint increment is sampled: etheta = 0),
# one increment (7), the benchmark's 11, the 64-row kernel (40), the HBM-workspace kernel (70)
PLAN_LENGTHS = (4, 5, 6, 7, 11, 40, 70)
VARIANTS = 9  # velocity triples per plan: 72 robots, two blocks, every plan in every wavefront
TWO_PI = 2.0 * np.pi

# name: (robot x, y, yaw; path start x, y; path heading).  The path is straight, 5 m long.
STRAIGHT = {
    # y (resp. x) is one constant: gy == 0 (resp. gx == 0) exactly, so etheta is 0 although the
    # robot's yaw is 0.3 off the path's heading
    "along_x": ((0.3, -0.2, 0.3), (0.5, 0.1), 0.0),
    "along_y": ((-0.4, 0.2, 0.5 * np.pi - 0.3), (-0.25, 0.3), 0.5 * np.pi),
    # yaw <= -pi + heading: yaw + 2 pi - heading = 2 pi - 6 = 0.2832
    "wrap": ((1.0, 1.0, -3.0), (1.1, 0.8), 3.0),
    # yaw - heading = 6 >= 1.8 pi: etheta = 0
    "cutoff": ((1.0, 1.0, 3.0), (1.1, 0.8), -3.0),
    # the whole path at x < 0 of the vehicle frame: from 6 m to 1 m behind the robot
    "behind": ((0.0, 0.0, 0.2), (-6.0 * np.cos(0.1) - 0.02, -6.0 * np.sin(0.1) + 0.2), 0.1),
    # 5 m to the left of a path it is turned 0.6 away from: cte = -5 / cos(0.6) = -6.06
    "beside": ((1.5 * np.cos(0.25) - 5.0 * np.sin(0.25) - 1.0, 1.5 * np.sin(0.25) + 5.0 * np.cos(0.25), 0.85),
               (-1.0, 0.0), 0.25),
    # facing backwards along the path: etheta = 2.94 - 0.3 = 2.64
    "backwards": ((1.5 * np.cos(0.3), 1.5 * np.sin(0.3) + 0.1, 2.94), (0.0, 0.0), 0.3),
}
NAMES = tuple(STRAIGHT) + ("circle",)  # a circle of radius 0.5 m, 3 m of arc from the robot's feet


def robots(M: int):
    """(pose [B, 3], vel [B, 3], plan [B, M, 2], name of robot b) for B = VARIANTS * len(NAMES):
    robot b follows plan NAMES[b % 8] with the velocity triple b // 8."""
    rng = np.random.default_rng(11)
    vels = np.stack([rng.uniform(0.0, 0.8, VARIANTS), rng.uniform(-1.0, 1.0, VARIANTS),
                     rng.uniform(-1.0, 1.0, VARIANTS)], axis=1)
    vels[0] = (0.5, 0.0, 0.0)
    pose1, plan1 = [], []
    s = np.linspace(0.0, 5.0, M)
    for name in NAMES:
        if name == "circle":
            a = np.linspace(0.0, 3.0, M) / 0.5
            pose1.append((0.05, -0.05, 0.1))
            plan1.append(np.stack([0.5 * np.sin(a), 0.5 - 0.5 * np.cos(a)], axis=1))
            continue
        pose, (x0, y0), h = STRAIGHT[name]
        pose1.append(pose)
        # (an axis-aligned path keeps its constant coordinate bit for bit)
        px = np.full(M, x0) if name == "along_y" else x0 + s * np.cos(h)
        py = np.full(M, y0) if name == "along_x" else y0 + s * np.sin(h)
        plan1.append(np.stack([px, py], axis=1))
    n = len(NAMES)
    B = VARIANTS * n
    pose = np.array([pose1[b % n] for b in range(B)], dtype=np.float64)
    plan = np.array([plan1[b % n] for b in range(B)], dtype=np.float64)
    vel = np.array([vels[b // n] for b in range(B)], dtype=np.float64)
    return pose, vel, plan, [NAMES[b % n] for b in range(B)]


def heading_sums(plan_b, M=None):
    """(gx, gy) of one robot's plan, in findBestPath's order of additions."""
    M = len(plan_b) if M is None else M
    gx = gy = 0.0
    for i in range(1, int(M * 0.3)):
        gx += plan_b[i, 0] - plan_b[i - 1, 0]
        gy += plan_b[i, 1] - plan_b[i - 1, 1]
    return gx, gy


def assert_branches(M, pose, plan, names, state_nodelay):
    """On the reference's output without delay mode (state[4] = cte, state[5] = etheta): every robot
    takes the branch its plan is named for.  Returns the names of the branches seen."""
    seen = set()
    for b, name in enumerate(names):
        gx, gy = heading_sums(plan[b], M)
        yaw, cte, eth = pose[b, 2], state_nodelay[b, 4], state_nodelay[b, 5]
        traj = np.arctan2(gy, gx)
        if int(M * 0.3) <= 1:
            assert gx == 0.0 and gy == 0.0 and eth == 0.0, (M, name)
            seen.add("no_increment")
        elif name == "along_x":
            assert gy == 0.0 and gx > 0.0 and eth == 0.0 and yaw - traj == 0.3, (M, name)
            seen.add("gy_zero")
        elif name == "along_y":
            assert gx == 0.0 and gy > 0.0 and eth == 0.0 and abs(yaw - traj + 0.3) < 1e-12, (M, name)
            seen.add("gx_zero")
        elif name == "wrap":
            assert yaw <= -np.pi + traj and abs(eth - (TWO_PI - 6.0)) < 1e-9, (M, name, eth)
            seen.add("wrap")
        elif name == "cutoff":
            assert not yaw <= -np.pi + traj and yaw - traj >= 1.8 * np.pi and eth == 0.0, (M, name, eth)
            seen.add("cutoff")
        elif name == "backwards":
            assert abs(eth - 2.64) < 1e-9, (M, name, eth)
            seen.add("backwards")
        if name == "beside":
            assert abs(cte + 5.0 / np.cos(0.6)) < 1e-6, (M, name, cte)
            seen.add("beside")
        if name == "behind":
            c, s = np.cos(yaw), np.sin(yaw)
            assert ((plan[b, :, 0] - pose[b, 0]) * c + (plan[b, :, 1] - pose[b, 1]) * s < -0.9).all()
            seen.add("behind")
    return seen
