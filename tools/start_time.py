#!/usr/bin/env python
"""Time a solve started from the previous tick's solution against the cold solve (DESIGN.md
"Start point in").

    python tools/start_time.py [--case cold,primal,full,shifted] [--batch 4096] [--ticks 6]
                               [--mu0 1e-2,1e-3,1e-4,1e-5,1e-6] [--steps 10] [--warmup 2] [--tag NAME]
                               [--shift-batch 65536] [--out profiles/start/times.jsonl]

B robots on the lemniscate (a dense course, standing start, offsets varied by robot) run --ticks
control ticks of the closed loop on the device (rollout).  The inputs of the last two ticks, k and
k + 1, are rebuilt from the rollout's logs (plan window, preprocessing, the robot's REF_V row).
Tick k is solved cold for its solution records; tick k + 1 is then solved cold, from tick k's
record as it is in PRIMAL mode, and in FULL mode at each --mu0; with `shifted` also from tick k's
record carried to tick k + 1 (mpcg_shift_solution_device with the motion between the two logged
poses, the rollout's formula evaluated by torch on the device), PRIMAL and FULL alike.  One JSON line
is printed and appended to --out: per case the total iterations, the share of status 1, the largest
|u0 - cold u0|, the robots whose u0 differs from the cold solve's by more than 1e-6 (another local
minimum) and the mean / min / max milliseconds per batch over --steps timed solves (HIP events on
the solve's stream around the call; device-resident inputs, workspace reserved; the cases take
turns, one solve each per round, so all see the same neighbours on the machine).  The shift itself
is not in a case's time; --shift-batch times the shift kernel alone (0: not), out of place on random
records of that many robots at the same horizon: the median of --steps x 4 calls, and its traffic of
2 x (30N - 6) x 8 bytes per robot as a rate.  Run it several times for the run-to-run spread.  The case `cold` uses only entry points the library had before the start point,
so the same file times an older checkout (copy it there; --tag names the build).
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

WINDOW_WP, STRIDE = 100, 10  # a 5 m window of the 0.05 m course, the reference's down-sampling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="cold,primal,full,shifted")
    ap.add_argument("--shift-batch", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=6)
    ap.add_argument("--mu0", default="1e-2,1e-3,1e-4,1e-5,1e-6")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "start", "times.jsonl"))
    a = ap.parse_args()
    if a.ticks < 2:
        sys.exit("--ticks must be at least 2")
    import torch

    from mpc_ros_amd import build, closed_loop, infinity, params
    from mpc_ros_amd.solver import BatchSolver, solution_elems

    dev = torch.device("cuda", 0)
    B, K = a.batch, a.ticks
    P = dict(params.PLUGIN_DEFAULTS)
    N = int(P["STEPS"])
    s = BatchSolver(0, P)
    course = closed_loop.course_infinity()
    arc = infinity._arc()
    pose, cursor = np.zeros((B, 3)), np.zeros(B, dtype=np.int32)
    for b in range(B):
        t0 = 0.3 + 5.4 * b / B
        lateral, heading_err = 0.15 * np.cos(1.0 * b), 0.2 * np.sin(1.3 * b)
        x, y = arc.point(t0)
        hd = float(arc.heading(t0))
        yaw = hd + heading_err
        pose[b] = (x - np.sin(hd) * lateral, y + np.cos(hd) * lateral, np.arctan2(np.sin(yaw), np.cos(yaw)))
        cursor[b] = max(int(arc.s_at(t0) / closed_loop.COURSE_SPACING) - 3, 0)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    courses, lens, course_of = up(course[None]), up(np.array([len(course)], dtype=np.int32)), up(np.zeros(B, dtype=np.int32))
    st = dict(pose=up(pose), vel=up(np.zeros((B, 3))), cursor=up(cursor), ref_v=up(np.full(B, float(P["REF_V"]))),
              done=up(np.zeros(B, dtype=np.int32)))
    logs = s.rollout_logs(K, B, names=("pose", "vel", "cursor", "ref_v", "count"))
    s.rollout(K, courses, lens, course_of, WINDOW_WP, STRIDE, st["pose"], st["vel"], st["cursor"], st["ref_v"],
              st["done"], logs=logs)
    torch.cuda.synchronize()
    mmax = closed_loop.plan_window_mmax(WINDOW_WP, STRIDE)

    def tick_inputs(k):
        """(state, coeffs, rows) of tick k, as the rollout's tick built them."""
        cur = logs["cursor"][k - 1].clone() if k > 0 else up(cursor)
        plan = torch.zeros((B, mmax, 2), dtype=torch.float64, device=dev)
        count = torch.zeros(B, dtype=torch.int32, device=dev)
        pk = logs["pose"][k].contiguous()
        s.plan_window_device(courses, lens, course_of, pk, WINDOW_WP, STRIDE, cur, plan, count)
        state = torch.empty((B, 6), dtype=torch.float64, device=dev)
        coeffs = torch.empty((B, 4), dtype=torch.float64, device=dev)
        s.preprocess_device(pk, logs["vel"][k].contiguous(), plan, state, coeffs, count=count)
        torch.cuda.synchronize()
        rows = up(params.rows(P, REF_V=logs["ref_v"][k].cpu().numpy()))
        return state, coeffs, rows

    run = st["done"].cpu().numpy() == 0  # (robots still running after the last tick)
    s0, c0, r0 = tick_inputs(K - 2)
    s1, c1, r1 = tick_inputs(K - 1)
    s.reserve(B)
    ne = solution_elems(N)
    rec = torch.zeros((B, ne), dtype=torch.float64, device=dev)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    used = torch.empty(B, dtype=torch.int32, device=dev)
    sol = torch.empty((B, ne), dtype=torch.float64, device=dev)
    s.solve_device(s0, c0, u0, status=status, iters=iters, pparams=r0, sol=rec)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    want = a.case.split(",")
    # tick k's records carried to tick k + 1: the motion between the two logged poses
    rec_sh = None
    if "shifted" in want:  # (entry points an older checkout does not have)
        p0, p1 = logs["pose"][K - 2], logs["pose"][K - 1]
        dX, dY, dpsi = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
        cs0, sn0 = torch.cos(p0[:, 2]), torch.sin(p0[:, 2])
        motion = torch.stack([cs0 * dX + sn0 * dY, -sn0 * dX + cs0 * dY, torch.atan2(torch.sin(dpsi), torch.cos(dpsi))],
                             dim=1).contiguous()
        rec_sh = torch.empty_like(rec)
        s.shift_solution_device(s1, c1, motion, rec, rec_sh, pparams=r1)
        torch.cuda.synchronize()
    cases = [("cold", None, None, None)]  # (always: the other cases' u0 is compared with it)
    starts = [("", rec)] + ([("_shifted", rec_sh)] if "shifted" in want else [])
    for suffix, start in starts:
        if "primal" in want:
            cases.append(("primal" + suffix, 1, None, start))  # MPCG_START_PRIMAL
        if "full" in want:
            cases += [(f"full{suffix}_mu0_{m}", 2, float(m), start) for m in a.mu0.split(",")]  # MPCG_START_FULL
    calls = []
    for name, mode, m0, start in cases:
        if mode is None:
            call = lambda: s.solve_device(s1, c1, u0, status=status, iters=iters, pparams=r1, sol=sol,  # noqa: E731
                                          stream=stream)
        else:
            tm = torch.full((B,), mode, dtype=torch.int32, device=dev)
            tmu = None if m0 is None else torch.full((B,), m0, dtype=torch.float64, device=dev)
            call = lambda tm=tm, tmu=tmu, start=start: s.solve_device(  # noqa: E731
                s1, c1, u0, status=status, iters=iters, pparams=r1, sol=sol, start=start, start_mode=tm, mu0=tmu,
                start_used=used, stream=stream)
        calls.append(call)
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    evs = [[] for _ in cases]
    for _ in range(a.steps):  # (the cases take turns)
        for ev, call in zip(evs, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            ev.append((e0, e1))
    torch.cuda.synchronize()
    out, u_cold = [], None
    for (name, mode, m0, start), call, ev in zip(cases, calls, evs):
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        call()  # (once more for this case's outputs)
        torch.cuda.synchronize()
        u = u0.cpu().numpy()
        if u_cold is None:
            u_cold = u.copy()
        it, stt = iters.cpu().numpy(), status.cpu().numpy()
        out.append(dict(case=name, kernel=s.last_kernel, iters_total=int(it[run].sum()), status_ok=float((stt[run] == 1).mean()),
                        used_ok=None if mode is None else float((used.cpu().numpy()[run] == mode).mean()),
                        max_du0=float(np.abs(u - u_cold)[run].max()),
                        other_minimum=int((np.abs(u - u_cold)[run].max(axis=1) > 1e-6).sum()), ms_mean=float(np.mean(ms)),
                        ms_min=float(np.min(ms)), ms_max=float(np.max(ms))))
    shift = None
    if a.shift_batch > 0 and "shifted" in want:
        Bs = a.shift_batch
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device=dev, generator=g) - 0.5  # noqa: E731
        a_in, a_out = rnd(Bs, ne), torch.empty((Bs, ne), dtype=torch.float64, device=dev)
        sst, scf, smo = rnd(Bs, 6), rnd(Bs, 4), 0.2 * rnd(Bs, 3)
        for _ in range(a.warmup):
            s.shift_solution_device(sst, scf, smo, a_in, a_out, stream=stream)
        ev = []
        for _ in range(4 * a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.shift_solution_device(sst, scf, smo, a_in, a_out, stream=stream)
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        nbytes = 2 * (30 * N - 6) * 8 * Bs
        shift = dict(B=Bs, N=N, calls=len(ms), ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                     ms_max=float(np.max(ms)), bytes=nbytes, tb_per_s=float(nbytes / (np.median(ms) * 1e-3) / 1e12))
    line = json.dumps(dict(tool="start_time", tag=a.tag, B=B, N=N, ticks=K, running=int(run.sum()), steps=a.steps,
                           build_id=build.built_id(), cases=out, shift_kernel=shift))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
