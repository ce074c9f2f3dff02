"""Closed-loop single robot on the infinity course (BASELINE configs[0]).

The reference's tracking loop (mpc_ros/src/driving_state.cpp:175-269): every control
tick the robot's pose and feedback speed, the previous command (_w, _throttle) and the
next waypoints of the plan go through findBestPath's preprocessing and MPC::Solve; the
post-processing turns (w0, a0) into the command speed = min(v + a0 dt, REF_V), and the
command is fed back (driving_state.cpp:191-193, 262-269).  Here the "robot" is the
unicycle the NLP models, integrated over one control period per tick, and the plan is
the next 5 m of the lemniscate (infinity.py), so the whole loop is reproducible.

`step_fn(pose[3], vel[3], plan[M,2]) -> cmd[3]` is one control tick (the GPU's
mpcg_track_device at B = 1, or a checker's restatement).
"""
from __future__ import annotations

import numpy as np

from . import infinity


def nearest_t(px: float, py: float, t_prev: float, window: float = 0.6, n: int = 601) -> float:
    """Path parameter of the closest lemniscate point near the previous one (forward search)."""
    arc = infinity._arc()
    ts = t_prev + np.linspace(-0.1 * window, window, n)
    x, y = arc.point(ts)
    return float(ts[np.argmin((x - px) ** 2 + (y - py) ** 2)])


def plan_from(t: float) -> np.ndarray:
    """The next PATH_LENGTH metres of the course from parameter t: [M, 2] waypoints."""
    arc = infinity._arc()
    s0 = float(np.interp(t % (4.0 * np.pi), arc.t, arc.s))
    ds = infinity.PATH_LENGTH / (infinity.N_WAYPOINTS - 1)
    tj = arc.t_at(s0 + ds * np.arange(infinity.N_WAYPOINTS))
    wx, wy = arc.point(tj)
    return np.stack([wx, wy], axis=-1)


def run(step_fn, ticks: int = 200, dt: float = 0.1, t0: float = 0.3, lateral: float = 0.15,
        heading_err: float = 0.2) -> dict:
    """Drive `ticks` control periods from a pose offset from the course; returns the
    per-tick pose, feedback and command arrays."""
    arc = infinity._arc()
    x, y = arc.point(t0)
    hd = float(arc.heading(t0))
    x, y = float(x - np.sin(hd) * lateral), float(y + np.cos(hd) * lateral)
    yaw = hd + heading_err
    v, w_prev, a_prev, t = 0.0, 0.0, 0.0, t0
    poses, cmds, cte = [], [], []
    for _ in range(ticks):
        t = nearest_t(x, y, t)
        plan = plan_from(t)
        pose = np.array([x, y, np.arctan2(np.sin(yaw), np.cos(yaw))])
        vel = np.array([v, w_prev, a_prev])
        cmd = np.asarray(step_fn(pose, vel, plan), dtype=np.float64)  # speed, w, throttle
        poses.append(pose)
        cmds.append(cmd)
        px, py = arc.point(t)
        cte.append(float(np.hypot(px - x, py - y)))
        speed, w, a = float(cmd[0]), float(cmd[1]), float(cmd[2])
        # the unicycle over one control period with the commanded speed and turn rate
        x += speed * np.cos(yaw) * dt
        y += speed * np.sin(yaw) * dt
        yaw += w * dt
        v, w_prev, a_prev = speed, w, a
    return dict(pose=np.array(poses), cmd=np.array(cmds), dist=np.array(cte))


# ---- the closed loop on the device (mpcg_rollout_device): dense courses and their window ----
COURSE_SPACING = 0.05  # metres between the waypoints of a dense course (a global planner's plan)


def course_infinity(laps: float = 1.0, spacing: float = COURSE_SPACING) -> np.ndarray:
    """The lemniscate as a dense global plan: [G, 2] waypoints every `spacing` metres of arc
    from t = 0 over `laps` rounds.  The arc length is integrated by Simpson's rule here (the
    benchmark's trapezoid table is 8e-11 m long on the first segment, where the course is
    straight to third order: a chord of 0.05 m + 8e-11 would turn the reference's
    int(path_length / 10 / dist) from 10 into 9)."""
    A = infinity.LEMNISCATE_A
    n = 20000 * max(1, int(np.ceil(laps)))
    t = np.linspace(0.0, 2.0 * np.pi * max(1, int(np.ceil(laps))), n + 1)
    speed = lambda u: np.hypot(A * np.cos(u), A * np.cos(2.0 * u))  # noqa: E731
    seg = (t[1] - t[0]) / 6.0 * (speed(t[:-1]) + 4.0 * speed(0.5 * (t[:-1] + t[1:])) + speed(t[1:]))
    arc_s = np.concatenate([[0.0], np.cumsum(seg)])
    total = float(np.interp(2.0 * np.pi * laps, t, arc_s))
    s = spacing * np.arange(int(np.floor(total / spacing)) + 1)
    tj = np.interp(s, arc_s, t)
    i = np.clip(np.searchsorted(t, tj, side="right") - 1, 0, n - 1)
    for _ in range(2):  # Newton on s(t) = s_j from the table's node below (the table is linear between nodes)
        h = tj - t[i]
        s_at = arc_s[i] + h / 6.0 * (speed(t[i]) + 4.0 * speed(t[i] + 0.5 * h) + speed(tj))
        tj = tj - (s_at - s) / speed(tj)
    return np.stack([A * np.sin(tj), A * np.sin(tj) * np.cos(tj)], axis=-1)


def course_straight(length: float, spacing: float = COURSE_SPACING, origin=(0.0, 0.0), heading: float = 0.0) -> np.ndarray:
    """A straight course of `length` metres from `origin` along `heading`: [G, 2] waypoints."""
    s = spacing * np.arange(int(round(length / spacing)) + 1)
    return np.stack([origin[0] + s * np.cos(heading), origin[1] + s * np.sin(heading)], axis=-1)


def stride_from(path_length: float, course: np.ndarray) -> int:
    """The reference's _downSampling (mpc_planner_ros.cpp:371-374): int(path_length / 10 /
    hypot(wp1 - wp0)), every stride-th waypoint of the window goes to the solver's plan."""
    d = float(np.hypot(course[1, 0] - course[0, 0], course[1, 1] - course[0, 1]))
    return int(path_length / 10.0 / d)


def plan_window_mmax(window_wp: int, stride: int) -> int:
    """Rows of a robot's sampled plan: ceil(window_wp / stride) + 1 (mpcg_plan_window_mmax)."""
    from . import _lib

    return _lib.check(_lib.lib().mpcg_plan_window_mmax(int(window_wp), int(stride)), "mpcg_plan_window_mmax")


def plan_window(course: np.ndarray, cursor: int, x: float, y: float, window_wp: int, stride: int):
    """One robot's plan window on the host (mpcg_plan_window, the code the kernel runs):
    getCutOffPlan from `cursor` at (x, y), window_wp waypoints, every stride-th and the last one
    once more.  Returns (new_cursor, start, count, plan [Mmax, 2]); rows past count are 0."""
    import ctypes as C

    from . import _lib

    course = np.ascontiguousarray(course, dtype=np.float64)
    assert course.ndim == 2 and course.shape[1] == 2
    mmax = _lib.lib().mpcg_plan_window_mmax(int(window_wp), int(stride))
    plan = np.zeros((max(mmax, 1), 2))
    out = [C.c_int32() for _ in range(3)]
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.lib().mpcg_plan_window(course.ctypes.data_as(dp), course.shape[0], int(cursor), float(x), float(y),
                                           int(window_wp), int(stride), *(C.byref(o) for o in out),
                                           plan.ctypes.data_as(dp)), "mpcg_plan_window")
    return out[0].value, out[1].value, out[2].value, plan
