#!/usr/bin/env python
"""Time the per-problem solve against the plain one (DESIGN.md "Per-problem parameters").

    python tools/pp_time.py [--case plain,pp_uniform,pp_mixed,track,track_goal] [--batch 65536]
                            [--horizon 20] [--model diffdrive|bicycle] [--steps 20] [--warmup 3] [--tag NAME]
                            [--out profiles/pp/times.jsonl]

One JSON line per case is appended to --out and printed: the mean / min / max over --steps timed
solves in milliseconds, HIP events on the solve's stream around the call, as bench.py times it
(device-resident inputs, workspace reserved).  Run it several times for the run-to-run spread.
The cases `plain` and `track` use only entry points the library had before the per-problem
ones, so the same file times an older checkout (copy it there; --tag names the build).

  plain       solve_device, the handle's parameters
  plain_general  the same on the general-options instance (an inert option changed): the plain
              twin of a general-options per-problem instance
  pp_uniform  solve_device with a row per problem, every row the handle's parameters
  pp_general  the same on the general-options per-problem instance (the inert option again)
  pp_mixed    the same with REF_V per robot uniform in [0.05, 1]
  track       track_device (preprocessing, solve, post-processing)
  track_goal  track_device with goals and ref_v (deceleration first, a row per robot); the goals
              lie 10 m away, so REF_V stays the handle's and the solves are those of `track`
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="plain,pp_uniform,pp_mixed,track,track_goal")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--model", default="diffdrive", choices=("diffdrive", "bicycle"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pp", "times.jsonl"))
    a = ap.parse_args()
    import torch

    from mpc_ros_amd import build, params
    from mpc_ros_amd.solver import BatchSolver

    dev = torch.device("cuda", 0)
    B, N = a.batch, a.horizon
    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    if a.model == "bicycle":  # (bench.py's bicycle: steering bound 0.5 rad, wheelbase 0.5 m)
        P.update(MODEL=1, LF=0.5, ANGVEL=0.5)
    s = BatchSolver(0, P)
    pose, vel, plan = s.synth_infinity_device(0, B)
    st = torch.empty((B, 6), dtype=torch.float64, device=dev)
    cf = torch.empty((B, 4), dtype=torch.float64, device=dev)
    s.preprocess_device(pose, vel, plan, st, cf)
    s.reserve(B)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    traj = torch.empty((B, 3, N), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    diag = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    cmd = torch.empty((B, 3), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    torch.cuda.synchronize()

    def rows_for(case):
        rng = np.random.default_rng(1)
        if case == "pp_uniform":
            return torch.from_numpy(params.rows(P, B=B)).to(dev)
        return torch.from_numpy(params.rows(P, REF_V=rng.uniform(0.05, 1.0, B))).to(dev)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for case in a.case.split(","):
        if case in ("plain_general", "pp_general"):
            s.set_params(P, acceptable_obj_change_tol=1e30)
        if case in ("plain", "plain_general"):
            call = lambda: s.solve_device(st, cf, u0, traj, status, None, iters, stream=stream, diag=diag)  # noqa: E731
        elif case in ("pp_uniform", "pp_general", "pp_mixed"):
            rows = rows_for("pp_mixed" if case == "pp_mixed" else "pp_uniform")
            call = lambda: s.solve_device(st, cf, u0, traj, status, None, iters, stream=stream, diag=diag,  # noqa: E731
                                          pparams=rows)
        elif case == "track":
            call = lambda: s.track_device(pose, vel, plan, cmd, traj, status, stream=stream)  # noqa: E731
        elif case == "track_goal":
            goal = (pose[:, :2] + 10.0).contiguous()
            ref_v = torch.full((B,), float(P["REF_V"]), dtype=torch.float64, device=dev)
            call = lambda: s.track_device(pose, vel, plan, cmd, traj, status, stream=stream, goal=goal,  # noqa: E731
                                          ref_v=ref_v)
        else:
            sys.exit(f"unknown case {case!r}")
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ev = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        rec = dict(case=case, tag=a.tag, model=a.model, B=B, N=N, steps=a.steps, ms_mean=float(np.mean(ms)), ms_min=float(np.min(ms)),
                   ms_max=float(np.max(ms)), kernel=s.last_kernel, build_id=build.built_id(),
                   iters_mean=float(iters.float().mean().item()) if case != "track" and case != "track_goal" else None,
                   status_ok=float((status == 1).float().mean().item()))
        line = json.dumps(rec)
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        if case in ("plain_general", "pp_general"):
            s.set_params(P)


if __name__ == "__main__":
    main()
