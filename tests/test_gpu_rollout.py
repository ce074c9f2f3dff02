"""GPU: the closed loop on the device -- the plan window (mpcg_plan_window_device), the
preprocessing with a waypoint count per robot (mpcg_preprocess_device_n) and the K-tick rollout
(mpcg_rollout_device), against the host window function (tests/test_plan_window.py checks it
against the reference's text), mpcg_decelerate and the oracle.

The rollout is compared on the device loop's own logged inputs, tick by tick, as
tests/test_closed_loop.py does and for the reason it gives: two loops closed separately drift
apart at rounding level until a tick near a local-minimum boundary sends them to different minima.
Tolerances: windows, REF_V and everything copied are exact; the preprocessing at
tests/test_gpu_track.py's 1e-9 (the oracle's operation order, FMA contraction apart); a tick's
command within 1e-6 of the oracle's and its status equal (test_closed_loop's bound); the unicycle
step to 1e-12 (three products and a sum per coordinate, |pose| < 20).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_pparams import hypot_exact, oracle_rows

pytestmark = pytest.mark.gpu

WINDOW_WP, STRIDE = 100, 10  # a 5 m window of the 0.05 m course, the reference's down-sampling: Mmax = 11
GOAL_TOL = 0.25
VMAX, VMIN = 0.7, 0.05
B_LEM, B_LINE, K = 64, 32, 25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def pack_courses(courses):
    """[C, Gmax, 2] (rows past a course's length are NaN: never read) and the lengths."""
    gmax = max(len(c) for c in courses)
    out = np.full((len(courses), gmax, 2), np.nan)
    for i, c in enumerate(courses):
        out[i, :len(c)] = c
    return out, np.array([len(c) for c in courses], dtype=np.int32)


def host_window(course, cursor, x, y, wp=WINDOW_WP, stride=STRIDE):
    from mpc_ros_amd import closed_loop

    return closed_loop.plan_window(course, cursor, x, y, wp, stride)


# ------------------------------------------------------------------ 1. the plan window
def test_plan_window_device_equals_the_host_function(torch_cuda):
    """B = 130: three wavefronts, the last one partial; two courses of different length; per
    lane another cursor, place and course, windows cut short by the course end (counts 0, 2, 3),
    a robot beyond 1000 m, and robots whose course index or cursor is out of range."""
    torch = torch_cuda
    from mpc_ros_amd import closed_loop, params
    from mpc_ros_amd.solver import BatchSolver

    courses = [closed_loop.course_infinity(), closed_loop.course_straight(3.0, origin=(4.0, -1.0), heading=0.7)]
    packed, lens = pack_courses(courses)
    B = 130
    rng = np.random.default_rng(130)
    course_of = (np.arange(B) % 3 == 0).astype(np.int32)
    cursor = np.zeros(B, dtype=np.int32)
    pose = np.zeros((B, 3))
    for b in range(B):
        G = lens[course_of[b]]
        k = [0, G // 3, G - 25, G - 12, G - 2, G - 1][b % 6] if b % 7 else int(rng.integers(0, G))
        cursor[b] = max(k - int(rng.integers(0, 4)), 0)
        pose[b, :2] = courses[course_of[b]][k] + rng.uniform(-0.03, 0.03, 2)
    pose[5, :2] = (1500.0, 3.0)  # (nothing erased)
    cursor[17], cursor[64] = lens[course_of[17]], -1  # cursor == G, cursor < 0
    course_of[[33, 129]] = 2, -1  # no such course
    s = BatchSolver(0, params.PLUGIN_DEFAULTS)
    mmax = closed_loop.plan_window_mmax(WINDOW_WP, STRIDE)
    assert mmax == 11
    tcur = dev(torch, cursor)
    plan = torch.full((B, mmax, 2), 7.0, dtype=torch.float64, device="cuda:0")
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    s.plan_window_device(dev(torch, packed), dev(torch, lens), dev(torch, course_of), dev(torch, pose), WINDOW_WP, STRIDE,
                         tcur, plan, count)
    torch.cuda.synchronize()
    got_cur, got_plan, got_count = tcur.cpu().numpy(), plan.cpu().numpy(), count.cpu().numpy()
    bad = [17, 64, 33, 129]
    seen = set()
    for b in range(B):
        if b in bad:
            assert got_count[b] == 0 and got_cur[b] == cursor[b] and (got_plan[b] == 0).all(), b
            continue
        cur, start, n, hp = host_window(courses[course_of[b]], cursor[b], pose[b, 0], pose[b, 1])
        assert (got_cur[b], got_count[b]) == (cur, n), b
        assert got_plan[b].tobytes() == hp.tobytes(), b
        seen.add(n)
    assert {0, 2, 3, 11} <= seen, seen
    assert got_cur[5] == cursor[5] and got_count[5] > 0


# ------------------------------------------------------------------ 2. a count per robot
def _plans(rng, B, M, pose):
    s = np.linspace(0.0, 5.0, M)
    plan = np.empty((B, M, 2))
    for b in range(B):
        hd = rng.uniform(-np.pi, np.pi) + rng.uniform(-0.4, 0.4) * s
        plan[b, :, 0] = pose[b, 0] + rng.uniform(-0.3, 0.3) + np.cumsum(np.cos(hd)) * (s[1] - s[0])
        plan[b, :, 1] = pose[b, 1] + rng.uniform(-0.3, 0.3) + np.cumsum(np.sin(hd)) * (s[1] - s[0])
    return plan


@pytest.mark.parametrize("mmax", [16, 64])
def test_preprocess_with_a_count_per_robot_matches_oracle(torch_cuda, oracle, mmax):
    """Counts 4..Mmax in one batch (both instances of the kernel), each robot against
    ora_find_best_path with its own M; counts 0..3 are not fitted: zeros.  A uniform count
    reproduces mpcg_preprocess_device bitwise."""
    torch = torch_cuda
    from mpc_ros_amd import params
    from mpc_ros_amd.solver import BatchSolver

    rng = np.random.default_rng(mmax)
    counts = np.r_[np.arange(4, mmax + 1), np.arange(0, 4), np.arange(4, mmax + 1)[::-1]].astype(np.int32)
    B = len(counts)
    assert B > 64 or mmax == 16
    pose = np.stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
    vel = np.stack([rng.uniform(0, 0.8, B), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)], axis=1)
    plan = _plans(rng, B, mmax, pose)
    for b in range(B):
        plan[b, counts[b]:] = 1e3 * (b + 1)  # (rows past the count are not read: garbage there changes nothing)
    s = BatchSolver(0, params.PLUGIN_DEFAULTS)
    st = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda:0")
    cf = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda:0")
    tpose, tvel = dev(torch, pose), dev(torch, vel)
    for delay in (True, False):
        s.preprocess_device(tpose, tvel, dev(torch, plan), st, cf, delay_mode=delay, count=dev(torch, counts))
        torch.cuda.synchronize()
        gst, gcf = st.cpu().numpy(), cf.cpu().numpy()
        for b in range(B):
            if counts[b] < 4:
                assert (gst[b] == 0).all() and (gcf[b] == 0).all(), b
                continue
            rc, ost, ocf = oracle.find_best_path(*pose[b], *vel[b], 0.1, plan[b, :counts[b]], delay)
            assert rc == 0
            np.testing.assert_allclose(gcf[b], ocf, rtol=1e-9, atol=1e-9, err_msg=str(b))
            np.testing.assert_allclose(gst[b], ost, rtol=1e-9, atol=1e-9, err_msg=str(b))
    # a uniform count = the row stride: mpcg_preprocess_device, bitwise
    for m in {mmax, mmax - 5}:
        full = dev(torch, _plans(rng, B, m, pose))
        st2, cf2 = torch.empty_like(st), torch.empty_like(cf)
        s.preprocess_device(tpose, tvel, full, st, cf, count=dev(torch, np.full(B, m, dtype=np.int32)))
        s.preprocess_device(tpose, tvel, full, st2, cf2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cf.cpu().numpy(), cf2.cpu().numpy(), err_msg=f"coeffs, M = {m}")
        np.testing.assert_array_equal(st.cpu().numpy(), st2.cpu().numpy(), err_msg=f"state, M = {m}")


# ------------------------------------------------------------------ 3. the rollout
def scene():
    """96 robots on three courses: 64 on the lemniscate from closed_loop.run's offsets varied by
    robot index (standing start); 16 on a 3 m straight course of 0.05 m spacing, which they leave
    where fewer than 4 sampled waypoints remain (1 m before its end); 16 on a 3 m straight course
    of 0.01 m spacing, whose window reaches to 0.2 m before the end: these decelerate towards the
    goal and stop within GOAL_TOL of it.  (The lemniscate's last waypoint is its crossing point:
    a robot that passes the crossing within GOAL_TOL is at its goal by the rule, as it would be
    by the reference's isPositionReached.)"""
    from mpc_ros_amd import closed_loop, infinity

    courses = [closed_loop.course_infinity(),
               closed_loop.course_straight(3.0, origin=(10.0, 0.0), heading=0.5),
               closed_loop.course_straight(3.0, spacing=0.01, origin=(-10.0, 2.0), heading=-2.0)]
    arc = infinity._arc()
    B = B_LEM + B_LINE
    pose, vel = np.zeros((B, 3)), np.zeros((B, 3))
    cursor, course_of = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B_LEM):
        t0 = 0.3 + 0.085 * b
        lateral, heading_err = 0.15 * np.cos(1.0 * b), 0.2 * np.sin(1.3 * b)
        x, y = arc.point(t0)
        hd = float(arc.heading(t0))
        yaw = hd + heading_err
        pose[b] = (x - np.sin(hd) * lateral, y + np.cos(hd) * lateral, np.arctan2(np.sin(yaw), np.cos(yaw)))
        cursor[b] = max(int(arc.s_at(t0) / closed_loop.COURSE_SPACING) - 3, 0)
    for i in range(B_LINE):
        b = B_LEM + i
        c = 1 + i // 16
        j = i % 16
        hd = (0.5, -2.0)[c - 1]
        s0 = (1.0 + 0.05 * j) if c == 1 else (1.3 + 0.06 * j)
        lateral = 0.04 * np.cos(2.0 * j)
        o = courses[c][0]
        pose[b] = (o[0] + s0 * np.cos(hd) - np.sin(hd) * lateral, o[1] + s0 * np.sin(hd) + np.cos(hd) * lateral,
                   hd + 0.1 * np.sin(1.7 * j))
        vel[b] = (0.3 + 0.03 * j, 0.0, 0.0)
        course_of[b] = c
        cursor[b] = max(int(s0 / (0.05, 0.01)[c - 1]) - 5, 0)
    return dict(courses=courses, pose=pose, vel=vel, cursor=cursor, course_of=course_of, ref_v=np.full(B, 1.0),
                done=np.zeros(B, dtype=np.int32))


class Loop:
    """The scene on the device and a solver; run(K, ...) is one mpcg_rollout_device call on
    the current state, with fresh logs, returned as numpy arrays."""

    def __init__(self, torch, sc=None):
        from mpc_ros_amd import params
        from mpc_ros_amd.solver import BatchSolver

        self.torch, self.sc = torch, sc or scene()
        self.P = params.PLUGIN_DEFAULTS
        self.s = BatchSolver(0, self.P)
        packed, lens = pack_courses(self.sc["courses"])
        self.courses, self.lens, self.course_of = dev(torch, packed), dev(torch, lens), dev(torch, self.sc["course_of"])
        self.state = {k: dev(torch, self.sc[k]) for k in ("pose", "vel", "cursor", "ref_v", "done")}
        self.B = self.sc["pose"].shape[0]

    def restore(self):
        for k, t in self.state.items():
            t.copy_(self.torch.from_numpy(self.sc[k]))

    def call(self, K, logs, integrate=True, stream=None):
        st = self.state
        self.s.rollout(K, self.courses, self.lens, self.course_of, WINDOW_WP, STRIDE, st["pose"], st["vel"], st["cursor"],
                       st["ref_v"], st["done"], goal_tol=GOAL_TOL, max_speed=VMAX, min_speed=VMIN, integrate=integrate,
                       logs=logs, stream=stream)

    def run(self, K, integrate=True):
        logs = self.s.rollout_logs(K, self.B)
        for t in logs.values():
            t.fill_(-7)
        self.call(K, logs, integrate)
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in logs.items()}

    def final(self):
        return {k: v.cpu().numpy() for k, v in self.state.items()}


@pytest.fixture(scope="module")
def rolled(torch_cuda):
    """One K = 25 rollout of the scene: its logs and final state, shared by the tests below."""
    loop = Loop(torch_cuda)
    logs = loop.run(K)
    return dict(sc=loop.sc, P=loop.P, logs=logs, final=loop.final(), kernel=loop.s.last_kernel)


def running(done, k):
    """Robots still running at tick k (index): not done yet at that tick."""
    return (done == 0) | (done > k + 1)


def test_rollout_windows_and_ref_v_follow_the_host_functions(rolled, libmpcg):
    sc, lg, P = rolled["sc"], rolled["logs"], rolled["P"]
    B = sc["pose"].shape[0]
    cur_prev, rv_prev = sc["cursor"].copy(), sc["ref_v"].copy()
    np.testing.assert_array_equal(lg["pose"][0], sc["pose"])
    np.testing.assert_array_equal(lg["vel"][0], sc["vel"])
    goals = np.array([sc["courses"][c][-1] for c in sc["course_of"]])
    changed = 0
    for k in range(K):
        for b in range(B):
            cur, start, n, _ = host_window(sc["courses"][sc["course_of"][b]], cur_prev[b], lg["pose"][k, b, 0],
                                           lg["pose"][k, b, 1])
            assert (lg["cursor"][k, b], lg["start"][k, b], lg["count"][k, b]) == (cur, start, n), (k, b)
        dist = hypot_exact(lg["pose"][k, :, 0] - goals[:, 0], lg["pose"][k, :, 1] - goals[:, 1])
        want = np.array([libmpcg.mpcg_decelerate(dist[b], lg["vel"][k, b, 0], max(P["MAXTHR"], 0.1), VMAX, VMIN,
                                                 rv_prev[b]) for b in range(B)])
        np.testing.assert_array_equal(lg["ref_v"][k], want, err_msg=str(k))
        changed += int((want != rv_prev).sum())
        cur_prev, rv_prev = lg["cursor"][k], lg["ref_v"][k]
    assert changed >= 8  # (the deceleration rule acted)
    np.testing.assert_array_equal(rolled["final"]["cursor"], lg["cursor"][-1])
    np.testing.assert_array_equal(rolled["final"]["ref_v"], lg["ref_v"][-1])
    assert (np.diff(lg["cursor"].astype(np.int64), axis=0) >= 0).all() and (lg["cursor"][-1] > sc["cursor"]).sum() > 80


def test_rollout_done_robots(rolled):
    """Done at the first tick with fewer than 4 sampled waypoints or within GOAL_TOL of the goal;
    from then on cmd 0, iters 0, status 13, vel 0 and the pose frozen.  Every robot of the two
    straight courses finishes within the K ticks; those of the fine one by the distance to the
    goal, after the deceleration rule has rewritten their REF_V."""
    sc, lg, fin = rolled["sc"], rolled["logs"], rolled["final"]
    done = fin["done"]
    B = len(done)
    goals = np.array([sc["courses"][c][-1] for c in sc["course_of"]])
    dist = np.stack([hypot_exact(lg["pose"][k, :, 0] - goals[:, 0], lg["pose"][k, :, 1] - goals[:, 1]) for k in range(K)])
    for b in range(B):
        stop = (lg["count"][:, b] < 4) | (dist[:, b] <= GOAL_TOL)
        want = int(np.argmax(stop)) + 1 if stop.any() else 0
        assert done[b] == want, (b, done[b], want)
        if want:
            k0 = want - 1
            assert (lg["cmd"][k0:, b] == 0).all() and (lg["iters"][k0:, b] == 0).all()
            assert (lg["status"][k0:, b] == 13).all()
            assert (lg["pose"][k0:, b] == lg["pose"][k0, b]).all() and (fin["pose"][b] == lg["pose"][k0, b]).all()
            assert (lg["vel"][k0 + 1:, b] == 0).all() and (fin["vel"][b] == 0).all()
        assert (lg["iters"][:want - 1 if want else K, b] > 0).all()
    line = sc["course_of"] > 0
    assert (done[line] > 1).all() and (done[~line] == 0).sum() >= 40
    by_goal = [b for b in range(B) if done[b] and lg["count"][done[b] - 1, b] >= 4]
    by_count = [b for b in range(B) if done[b] and lg["count"][done[b] - 1, b] < 4]
    assert len(by_count) >= 16
    slowed = [b for b in by_goal if lg["ref_v"][done[b] - 1, b] < sc["ref_v"][b]]
    assert len(slowed) >= 1, (by_goal, slowed)  # (done by deceleration to the goal)
    assert set(by_goal) >= set(np.flatnonzero(sc["course_of"] == 2))
    assert rolled["kernel"].startswith("k_solve_wide_pp<")


def oracle_ticks(oracle, dicts, st, cf):
    """The oracle's solve of problem i under dicts[i]: the problems that share the most common
    REF_V (the robots far from their goals) as one batch on 16 threads, the others by
    oracle_rows, one call per distinct REF_V."""
    from test_gpu_parity import oracle_ref

    rv = np.array([d["REF_V"] for d in dicts])
    vals, n = np.unique(rv, return_counts=True)
    big = rv == vals[n.argmax()]
    out = oracle_rows(oracle, [d for d, b in zip(dicts, big) if not b], st[~big], cf[~big]) if (~big).any() else None
    main = oracle_ref(oracle, dicts[int(np.flatnonzero(big)[0])], st[big], cf[big], threads=16)
    ref = {k: np.zeros((len(dicts),) + main[k].shape[1:], dtype=main[k].dtype) for k in ("u0", "status", "iters")}
    for k in ref:
        ref[k][big] = main[k]
        if out is not None:
            ref[k][~big] = out[k]
    return ref


def test_rollout_commands_match_the_oracle_tick(rolled, oracle):
    """Per tick and running robot: ora_find_best_path on the logged pose, feedback and window
    (the logged count), the oracle's solve with the logged REF_V, the post-processing.

    Where a window holds fewer than 4 distinct waypoints -- 4 samples of which the last is
    back() once more, W = stride 2 + 1 -- the reference's cubic fit is rank-deficient: its
    fourth pivot is rounding noise or exactly 0, so the reference itself returns either noise
    coefficients or NaN (status 11) there, decided by the last bit.  Those robot-ticks have no
    defined answer; they are counted, and their command must be finite and within the bounds."""
    sc, lg, P = rolled["sc"], rolled["logs"], rolled["P"]
    done = rolled["final"]["done"]
    B = len(done)
    cur_prev = sc["cursor"].copy()
    rows, sts, cfs, dicts, singular = [], [], [], [], []
    for k in range(K):
        for b in np.flatnonzero(running(done, k)):
            _, _, n, plan = host_window(sc["courses"][sc["course_of"][b]], cur_prev[b], lg["pose"][k, b, 0],
                                        lg["pose"][k, b, 1])
            if len({tuple(p) for p in plan[:n]}) < 4:
                singular.append((k, b))
                continue
            rc, st, cf = oracle.find_best_path(*lg["pose"][k, b], *lg["vel"][k, b], P["DT"], plan[:n], True)
            assert rc == 0
            rows.append((k, b))
            sts.append(st)
            cfs.append(cf)
            dicts.append(dict(P, REF_V=float(lg["ref_v"][k, b])))
        cur_prev = lg["cursor"][k]
    assert len(rows) > 0.6 * K * B and len(singular) < 0.01 * K * B
    for k, b in singular:
        c = lg["cmd"][k, b]
        assert lg["count"][k, b] == 4 and np.isfinite(c).all(), (k, b, c)
        assert c[0] <= lg["ref_v"][k, b] and abs(c[1]) <= P["ANGVEL"] + 1e-6 and abs(c[2]) <= P["MAXTHR"] + 1e-6
    ref = oracle_ticks(oracle, dicts, np.array(sts), np.array(cfs))
    kk, bb = np.array(rows).T
    cmd, v = lg["cmd"][kk, bb], lg["vel"][kk, bb, 0]
    want = np.stack([np.minimum(v + ref["u0"][:, 1] * P["DT"], lg["ref_v"][kk, bb]), ref["u0"][:, 0], ref["u0"][:, 1]], 1)
    diff = np.abs(cmd - want).max(1)
    print(f"rollout: {len(rows)} robot-ticks ({len(singular)} rank-deficient windows apart), max |dcmd| "
          f"{np.nanmax(diff):.2e} at tick, robot {rows[int(np.nanargmax(diff))]}, same iteration count on "
          f"{100 * np.mean(lg['iters'][kk, bb] == ref['iters']):.1f} %")
    np.testing.assert_array_equal(lg["status"][kk, bb], ref["status"])
    assert (ref["status"] == 1).mean() > 0.95
    assert np.all(diff <= 1e-6), (rows[int(np.nanargmax(diff))], np.nanmax(diff))


def test_a_rollout_tick_is_the_goal_tick_on_its_window(torch_cuda, rolled):
    """Every tick k and every robot running at it (its window holds at least 4 waypoints, else it
    would be done): mpcg_track_device_goal on the logged pose and feedback, the host window's
    plan rows, the course's last waypoint as the goal and the REF_V entering the tick gives the
    logged command, REF_V and status, bytes for bytes.  The goal tick takes one M per call, so the
    robots of a tick are grouped by their count.  None is left out; some have their REF_V rewritten
    by the deceleration rule, some hold a window shorter than Mmax."""
    torch = torch_cuda
    from mpc_ros_amd import closed_loop
    from mpc_ros_amd.solver import BatchSolver

    sc, lg, P = rolled["sc"], rolled["logs"], rolled["P"]
    done = rolled["final"]["done"]
    goals = np.array([sc["courses"][c][-1] for c in sc["course_of"]])
    mmax = closed_loop.plan_window_mmax(WINDOW_WP, STRIDE)
    s = BatchSolver(0, P)
    cur_prev, rv_prev = sc["cursor"].copy(), sc["ref_v"].copy()
    compared = slowed = short = 0
    for k in range(K):
        run = np.flatnonzero(running(done, k))
        count = lg["count"][k]
        assert (count[run] >= 4).all(), k
        plans = {b: host_window(sc["courses"][sc["course_of"][b]], cur_prev[b], lg["pose"][k, b, 0], lg["pose"][k, b, 1])[3]
                 for b in run}
        for n in np.unique(count[run]):
            g = run[count[run] == n]
            cmd = torch.full((len(g), 3), 7.0, dtype=torch.float64, device="cuda:0")
            status = torch.full((len(g),), -7, dtype=torch.int32, device="cuda:0")
            ref_v = dev(torch, rv_prev[g])
            s.track_device(dev(torch, lg["pose"][k, g]), dev(torch, lg["vel"][k, g]),
                           dev(torch, np.stack([plans[b][:n] for b in g])), cmd, status=status, goal=dev(torch, goals[g]),
                           ref_v=ref_v, max_speed=VMAX, min_speed=VMIN, delay_mode=True)
            torch.cuda.synchronize()
            assert ref_v.cpu().numpy().tobytes() == np.ascontiguousarray(lg["ref_v"][k, g]).tobytes(), (k, n)
            assert cmd.cpu().numpy().tobytes() == np.ascontiguousarray(lg["cmd"][k, g]).tobytes(), (k, n)
            assert status.cpu().numpy().tobytes() == np.ascontiguousarray(lg["status"][k, g]).tobytes(), (k, n)
        compared += len(run)
        slowed += int((lg["ref_v"][k, run] != rv_prev[run]).sum())
        short += int((count[run] < mmax).sum())
        cur_prev, rv_prev = lg["cursor"][k], lg["ref_v"][k]
    assert compared == sum(int(running(done, k).sum()) for k in range(K)) and compared > 0.6 * K * len(done)
    assert slowed >= 1 and short >= 1, (slowed, short)


def test_rollout_integrates_the_unicycle(rolled):
    sc, lg, P, fin = rolled["sc"], rolled["logs"], rolled["P"], rolled["final"]
    dt = P["DT"]
    nxt = np.concatenate([lg["pose"][1:], fin["pose"][None]])
    nvel = np.concatenate([lg["vel"][1:], fin["vel"][None]])
    x, y, yaw = lg["pose"][..., 0], lg["pose"][..., 1], lg["pose"][..., 2]
    speed, w = lg["cmd"][..., 0], lg["cmd"][..., 1]
    run = np.stack([running(fin["done"], k) for k in range(K)])
    yn = yaw + w * dt
    want = np.stack([x + speed * np.cos(yaw) * dt, y + speed * np.sin(yaw) * dt, np.arctan2(np.sin(yn), np.cos(yn))], -1)
    assert np.abs(nxt - want)[run].max() <= 1e-12
    np.testing.assert_array_equal(nxt[~run], lg["pose"][~run])  # (frozen)
    np.testing.assert_array_equal(nvel, lg["cmd"])  # (the command fed back; 0 for a done robot)
    assert np.abs(nxt - lg["pose"])[run].max() > 0.05  # (they move)


def test_rollout_state_carries_between_calls(torch_cuda, rolled):
    """One K = 6 rollout equals six K = 1 rollouts bitwise: state and logs; done holds the tick
    within its call, so in the six calls it is 1 in the call where the K = 6 rollout has k + 1."""
    a, b = Loop(torch_cuda, rolled["sc"]), Loop(torch_cuda, rolled["sc"])
    la = a.run(6)
    done_b = np.zeros(a.B, dtype=np.int32)
    for k in range(6):
        lb = b.run(1)
        for name in la:
            assert la[name][k].tobytes() == lb[name][0].tobytes(), (name, k)
        d = b.final()["done"]
        assert set(np.unique(d)) <= {0, 1}
        done_b[(done_b == 0) & (d == 1)] = k + 1
    fa, fb = a.final(), b.final()
    for name in ("pose", "vel", "cursor", "ref_v"):
        assert fa[name].tobytes() == fb[name].tobytes(), name
    np.testing.assert_array_equal(fa["done"], done_b)
    assert (fa["done"] > 1).any()
    for name in la:  # (and the first six ticks of the K = 25 rollout)
        assert la[name].tobytes() == rolled["logs"][name][:6].tobytes(), name


def test_real_robot_tick_leaves_the_pose_alone(torch_cuda, rolled):
    """integrate = 0, K = 1: the tick from a global plan.  Pose and feedback are the caller's; the
    command is the integrating tick's."""
    loop = Loop(torch_cuda, rolled["sc"])
    lg = loop.run(1, integrate=False)
    fin = loop.final()
    np.testing.assert_array_equal(fin["pose"], rolled["sc"]["pose"])
    np.testing.assert_array_equal(fin["vel"], rolled["sc"]["vel"])
    for name in lg:
        assert lg[name][0].tobytes() == rolled["logs"][name][0].tobytes(), name
    np.testing.assert_array_equal(fin["cursor"], rolled["logs"]["cursor"][0])
    np.testing.assert_array_equal(fin["ref_v"], rolled["logs"]["ref_v"][0])
    assert (np.abs(lg["cmd"][0]).max(1) > 0).sum() > 80


def test_rollout_in_a_captured_graph(torch_cuda, rolled):
    """K = 3 at B = 96 captured after one warm-up call on the capture stream, replayed twice from
    the restored inputs: every log and the final state bitwise the direct call's."""
    torch = torch_cuda
    loop = Loop(torch, rolled["sc"])
    want = {k: v[:3] for k, v in rolled["logs"].items()}
    logs = loop.s.rollout_logs(3, loop.B)
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        loop.call(3, logs, stream=side)  # (warm-up: the handle's buffers exist afterwards)
    torch.cuda.synchronize()
    direct_final = loop.final()
    loop.restore()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        loop.call(3, logs, stream=side)
    for _ in range(2):
        loop.restore()
        for t in logs.values():
            t.fill_(-7)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        for name, t in logs.items():
            assert t.cpu().numpy().tobytes() == want[name].tobytes(), name
        fin = loop.final()
        for name in fin:
            assert fin[name].tobytes() == direct_final[name].tobytes(), name


def test_rollout_refusals(torch_cuda, rolled):
    """K < 1, stride < 1, window_wp < 1, more than 64 sampled waypoints and the fp32 configuration
    are refused before anything is queued: the robots' state is untouched."""
    torch = torch_cuda
    from mpc_ros_amd import _lib, params
    from mpc_ros_amd.solver import BatchSolver

    loop = Loop(torch, rolled["sc"])
    st = loop.state

    def call(s, K=1, wp=WINDOW_WP, stride=STRIDE):
        s.rollout(K, loop.courses, loop.lens, loop.course_of, wp, stride, st["pose"], st["vel"], st["cursor"],
                  st["ref_v"], st["done"])

    for kw in (dict(K=0), dict(stride=0), dict(wp=0), dict(wp=64, stride=1), dict(wp=640, stride=10)):
        with pytest.raises(_lib.MpcgError):
            call(loop.s, **kw)
    with pytest.raises(_lib.MpcgError, match="fp32"):
        call(BatchSolver(0, params.PLUGIN_DEFAULTS, dtype="fp32"))
    plan = torch.zeros((loop.B, 65, 2), dtype=torch.float64, device="cuda:0")
    count = torch.zeros(loop.B, dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.MpcgError, match="64"):
        loop.s.plan_window_device(loop.courses, loop.lens, loop.course_of, st["pose"], 64, 1, st["cursor"], plan, count)
    torch.cuda.synchronize()
    fin = loop.final()
    for name in fin:
        np.testing.assert_array_equal(fin[name], rolled["sc"][name])
    call(loop.s, wp=63, stride=1)  # (Mmax = 64 is taken)
    torch.cuda.synchronize()
    assert C.sizeof(_lib.MpcgRolloutLogs) == 9 * C.sizeof(C.c_void_p)
