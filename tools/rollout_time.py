#!/usr/bin/env python
"""Time the K-tick rollout against the tick it replaces (DESIGN.md "Closed loop on the device").

    python tools/rollout_time.py [--batch 65536] [--horizon 20] [--ticks 20] [--repeats 7] [--warmup 2]
                                 [--goal-tol 0.1] [--tag NAME] [--out profiles/rollout/times.jsonl]

The robots are the benchmark's infinity set (pose offsets, speeds and previous commands of
infinity.draw_scenarios) on a dense lemniscate course of two laps, 0.05 m between waypoints, a
window of 100 waypoints sampled with the reference's stride 10: 11 waypoints per robot, the
benchmark's plan length, and no window is cut short by the course end within the ticks timed.

  rollout     one mpcg_rollout_device call of K ticks without logs, from the restored start state:
              HIP events on the stream around the call, divided by K.
  track_goal  the same K x B problems through mpcg_track_device_goal: a logged rollout gives every
              tick's pose and feedback; before each timed call the tick's plan is cut from the
              logged pose by mpcg_plan_window_device (untimed -- the host's work in the loop this
              replaces); HIP events around the K calls, summed, divided by K.  A robot that is done
              costs the rollout no iterations, while this path solves it again.

  warm        (--warm full; --mu0) the rollout with every tick started from the robot's
              previous solution, shifted to the tick (mpcg_rollout_device_start), timed as `rollout`
              from the restored start state and a carry zeroed before the events.  Per mode: ms per tick; the
              iterations summed over the robots, per tick, beside the cold rollout's (a logged run of
              each); the share of robot-ticks, over the robots running in both loops, whose command
              (w, a) differs from the cold loop's by more than 1e-6 -- another minimum, or a robot
              that an earlier one has put on another path -- and the share of robots with such a tick.
              The cold rollout's kernels are untouched by the warm path, so it is the baseline.

All are warmed up, then repeated alternately; the medians of the per-tick times, their ratios and
the share of robots done after K ticks go into one JSON line, appended to --out and printed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW_WP, STRIDE = 100, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--goal-tol", type=float, default=0.1)
    ap.add_argument("--warm", default="full")
    ap.add_argument("--mu0", type=float, default=1e-4)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout", "times.jsonl"))
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5 (the median of fewer says little)")
    import torch

    if not torch.cuda.is_available():
        sys.exit("rollout_time.py needs a GPU")
    from mpc_ros_amd import build, closed_loop, infinity, params
    from mpc_ros_amd.solver import BatchSolver

    dev = torch.device("cuda", 0)
    B, N, K = a.batch, a.horizon, a.ticks
    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    s = BatchSolver(0, P)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731

    course = closed_loop.course_infinity(laps=2.0)
    assert closed_loop.stride_from(infinity.PATH_LENGTH, course) == STRIDE
    mmax = closed_loop.plan_window_mmax(WINDOW_WP, STRIDE)
    sc = infinity.draw_scenarios(np.arange(B))
    px, py, yaw, _ = infinity.scenario_poses(sc)
    start = dict(pose=np.stack([px, py, yaw], 1), vel=np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], 1),
                 cursor=np.maximum((infinity._arc().s_at(sc["t"]) / closed_loop.COURSE_SPACING).astype(np.int32) - 3, 0),
                 ref_v=np.full(B, float(P["REF_V"])), done=np.zeros(B, dtype=np.int32))
    courses, lens = t(course[None]), t(np.array([len(course)], dtype=np.int32))
    course_of = torch.zeros(B, dtype=torch.int32, device=dev)
    goal = t(np.tile(course[-1], (B, 1)))
    state = {k: t(v) for k, v in start.items()}
    init = {k: v.clone() for k, v in state.items()}
    stream = torch.cuda.current_stream(dev)
    s.reserve(B)

    def restore():
        for k, v in state.items():
            v.copy_(init[k])

    def rollout(logs=None):
        s.rollout(K, courses, lens, course_of, WINDOW_WP, STRIDE, state["pose"], state["vel"], state["cursor"],
                  state["ref_v"], state["done"], goal_tol=a.goal_tol, logs=logs, stream=stream)

    # the logged rollout: every tick's inputs for the track_goal path
    logs = s.rollout_logs(K, B, names=("pose", "vel", "cursor", "ref_v", "count", "iters"))
    rollout(logs)
    torch.cuda.synchronize()
    kernel_cold = s.last_kernel
    done_share = float((state["done"] != 0).float().mean().item())
    full = float((logs["count"] == mmax).float().mean().item())
    cur_in = [init["cursor"]] + [logs["cursor"][k] for k in range(K - 1)]
    rv_in = [init["ref_v"]] + [logs["ref_v"][k] for k in range(K - 1)]
    plan = torch.empty((B, mmax, 2), dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    cursor = torch.empty(B, dtype=torch.int32, device=dev)
    ref_v = torch.empty(B, dtype=torch.float64, device=dev)
    cmd = torch.empty((B, 3), dtype=torch.float64, device=dev)

    modes = [(m, {"full": 2}[m]) for m in a.warm.split(",") if m]  # MPCG_START_FULL (PRIMAL is not offered)
    carry = s.rollout_carry(B) if modes else None

    def warm_rollout(mode, logs=None, used=None):  # (the caller has zeroed the carry)
        s.rollout(K, courses, lens, course_of, WINDOW_WP, STRIDE, state["pose"], state["vel"], state["cursor"],
                  state["ref_v"], state["done"], goal_tol=a.goal_tol, logs=logs, stream=stream, start_mode=mode,
                  mu0=a.mu0, carry=carry, log_start_used=used)

    def time_rollout(mode=None):
        restore()
        if mode is not None:
            for v in carry.values():
                v.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rollout() if mode is None else warm_rollout(mode)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K

    # a logged run of each mode against the cold loop's logs
    cold_cmd = None
    warm_stats = {}
    if modes:
        restore()
        lc = s.rollout_logs(K, B, names=("cmd", "iters"))
        rollout(lc)
        torch.cuda.synchronize()
        cold_cmd, cold_iters, cold_done = lc["cmd"].clone(), lc["iters"].sum(dim=1).tolist(), state["done"].clone()
        for name, mode in modes:
            restore()
            for v in carry.values():
                v.zero_()
            lw = s.rollout_logs(K, B, names=("cmd", "iters", "status"))
            used = torch.zeros((K, B), dtype=torch.int32, device=dev)
            warm_rollout(mode, lw, used)
            torch.cuda.synchronize()
            k_idx = torch.arange(K, device=dev)[:, None]
            both = ((cold_done[None] == 0) | (cold_done[None] > k_idx + 1)) & \
                   ((state["done"][None] == 0) | (state["done"][None] > k_idx + 1))
            diff = ((lw["cmd"][..., 1:] - cold_cmd[..., 1:]).abs().amax(dim=2) > 1e-6) & both
            warm_stats[name] = dict(iters_per_tick=lw["iters"].sum(dim=1).tolist(), cold_iters_per_tick=cold_iters,
                                    started_share=float(((used == mode) & both).sum().item() / max(both[1:].sum().item(), 1)),
                                    solved_share=float((((lw["status"] == 1) | (lw["status"] == 4)) & both).sum().item()
                                                       / max(both.sum().item(), 1)),
                                    other_minimum_tick_share=float(diff.sum().item() / max(both.sum().item(), 1)),
                                    other_minimum_robot_share=float(diff.any(dim=0).float().mean().item()),
                                    kernel=s.last_kernel)

    def time_track_goal():
        ev = []
        for k in range(K):
            cursor.copy_(cur_in[k])
            ref_v.copy_(rv_in[k])
            s.plan_window_device(courses, lens, course_of, logs["pose"][k], WINDOW_WP, STRIDE, cursor, plan, count,
                                 stream=stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.track_device(logs["pose"][k], logs["vel"][k], plan, cmd, stream=stream, goal=goal, ref_v=ref_v)
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / K

    for _ in range(a.warmup):
        time_rollout()
        time_track_goal()
        for _, mode in modes:
            time_rollout(mode)
    r_ms, g_ms, w_ms = [], [], {name: [] for name, _ in modes}
    for _ in range(a.repeats):  # (alternating: all see the same neighbours on the machine)
        r_ms.append(time_rollout())
        g_ms.append(time_track_goal())
        for name, mode in modes:
            w_ms[name].append(time_rollout(mode))
    for name, _ in modes:
        warm_stats[name].update(ms_per_tick=float(np.median(w_ms[name])),
                                ms_min_max=[float(min(w_ms[name])), float(max(w_ms[name]))],
                                ratio_to_cold=float(np.median(w_ms[name]) / np.median(r_ms)))
    rec = dict(tool="rollout_time", tag=a.tag, B=B, N=N, K=K, repeats=a.repeats, window_wp=WINDOW_WP, stride=STRIDE,
               goal_tol=a.goal_tol, rollout_ms_per_tick=float(np.median(r_ms)),
               track_goal_ms_per_tick=float(np.median(g_ms)),
               ratio=float(np.median(r_ms) / np.median(g_ms)), rollout_ms_min_max=[float(min(r_ms)), float(max(r_ms))],
               track_goal_ms_min_max=[float(min(g_ms)), float(max(g_ms))], done_share=done_share,
               full_window_share=full, iters_mean_first_tick=float(logs["iters"][0].float().mean().item()),
               iters_mean_last_tick=float(logs["iters"][K - 1].float().mean().item()), kernel=kernel_cold,
               mu0=a.mu0, warm=warm_stats, build_id=build.built_id())
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
