"""GPU: a solution record carried to the next tick -- the shift kernel (mpcg_shift_solution_device)
against the host function, the rollout started from each robot's previous record
(mpcg_rollout_device_start) on tests/test_gpu_rollout.py's 96-robot scene, and class MPC's
carry_motion.

Tolerances: the shift's mapped entries (a rotation, a difference, one step of the model; |values| <=
3 here) to 1e-12 against the host function, which differs from the kernel in sin / cos alone; every
entry that is only moved bit for bit.  A warm tick against the composition of the public device
calls on its logged inputs: the composition's motion is computed by torch on the device with the
rollout's formula, operation by operation, so the shifted record and with it u0, status and
iterations are bitwise; the speed min(v + a0 dt, REF_V) to 1e-15.

The rollout offers COLD and FULL; PRIMAL is refused (a PRIMAL tick is the composition of the public
calls, which test_cpp_class_carries_its_solution's Python side makes).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_rollout import GOAL_TOL, STRIDE, VMAX, VMIN, WINDOW_WP, Loop, dev, running, scene

pytestmark = pytest.mark.gpu

COLD, PRIMAL, FULL = 0, 1, 2
MU0 = 1e-4
K6 = 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


# ------------------------------------------------------------------ 1. the kernel against the host function
def mapped_mask(N):
    nx = 8 * N - 2
    m = np.zeros(3 * nx + 6 * N, dtype=bool)
    X = np.zeros((6, N), dtype=bool)
    X[:3, 1:N - 1] = True
    X[:, N - 1] = True
    m[:6 * N] = X.ravel()
    m[3 * nx:3 * nx + 2 * N] = True
    return m


@pytest.mark.parametrize("N,model", [(2, 0), (3, 0), (20, 0), (33, 0), (65, 0), (128, 0), (25, 1)])
def test_device_shift_equals_the_host_function(torch_cuda, N, model):
    """B = 70 (more than one block, the last problems behind a ragged mask), random finite records,
    motions with zero motion and headings near +-pi; with the handle's parameters and with a row
    per problem; in place equals out of place."""
    torch = torch_cuda
    from mpc_ros_amd import params, solver
    from mpc_ros_amd.solver import BatchSolver

    B = 70
    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    if model:
        P.update(MODEL=1, LF=0.4)
    rng = np.random.default_rng(70 + N)
    ne = solver.solution_elems(N)
    state, coeffs = rng.uniform(-0.5, 0.5, (B, 6)), rng.uniform(-0.3, 0.3, (B, 4))
    rec = rng.uniform(-3.0, 3.0, (B, ne))
    m = np.stack([rng.uniform(-0.1, 0.1, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.3, 0.3, B)], axis=1)
    m[0] = 0.0
    m[1], m[2], m[3] = (0.03, -0.01, np.pi - 1e-9), (-0.02, 0.04, -np.pi + 1e-9), (0.05, 0.02, np.pi)
    mask = (rng.uniform(size=B) < 0.7).astype(np.int32)
    mask[:4], mask[-1] = 1, 0
    rows = params.rows(P, DT=rng.uniform(0.05, 0.2, B))
    s = BatchSolver(0, P)
    tst, tcf, tm, trec, tmask, trows = (dev(torch, a) for a in (state, coeffs, m, rec, mask, rows))
    mapped = mapped_mask(N)
    for pp, hrows in ((None, None), (trows, rows)):
        for mk, hmask in ((None, None), (tmask, mask)):
            want = solver.shift_solution(dict(P), state, coeffs, m, rec, mask=hmask, params_rows=hrows)
            out = torch.full((B, ne), 7.0, dtype=torch.float64, device="cuda:0")
            s.shift_solution_device(tst, tcf, tm, trec, out, mask=mk, pparams=pp)
            inplace = trec.clone()
            s.shift_solution_device(tst, tcf, tm, inplace, inplace, mask=mk, pparams=pp)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            d = np.abs(got - want)
            print(f"N = {N}: max |device - host| on the mapped entries {d[:, mapped].max():.2e}")
            assert d[:, mapped].max() <= 1e-12
            assert got[:, ~mapped].tobytes() == want[:, ~mapped].tobytes()
            if hmask is not None:
                assert got[hmask == 0].tobytes() == rec[hmask == 0].tobytes()
            assert inplace.cpu().numpy().tobytes() == got.tobytes()
    assert trec.cpu().numpy().tobytes() == rec.tobytes()  # (the source of an out-of-place call is not written)


# ------------------------------------------------------------------ 2. the warm rollout
class WarmLoop(Loop):
    """test_gpu_rollout's Loop with a carry: run(K, mode) is one mpcg_rollout_device_start call."""

    def __init__(self, torch, sc=None):
        super().__init__(torch, sc)
        self.carry = self.s.rollout_carry(self.B)

    def restore(self):
        super().restore()
        for t in self.carry.values():
            t.zero_()

    def call_start(self, K, logs, used, mode, mu0=MU0, integrate=True, stream=None):
        st = self.state
        self.s.rollout(K, self.courses, self.lens, self.course_of, WINDOW_WP, STRIDE, st["pose"], st["vel"], st["cursor"],
                       st["ref_v"], st["done"], goal_tol=GOAL_TOL, max_speed=VMAX, min_speed=VMIN, integrate=integrate,
                       logs=logs, stream=stream, start_mode=mode, mu0=mu0, carry=self.carry, log_start_used=used)

    def run_start(self, K, mode, integrate=True):
        logs = self.s.rollout_logs(K, self.B)
        for t in logs.values():
            t.fill_(-7)
        used = self.torch.full((K, self.B), -7, dtype=self.torch.int32, device="cuda:0")
        self.call_start(K, logs, used, mode, integrate=integrate)
        self.torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in logs.items()}
        out["start_used"] = used.cpu().numpy()
        return out

    def final(self):
        out = super().final()
        out.update({"carry_" + k: v.cpu().numpy() for k, v in self.carry.items()})
        return out


@pytest.fixture(scope="module")
def sc():
    return scene()


@pytest.fixture(scope="module")
def cold6(torch_cuda, sc):
    """mpcg_rollout_device, K = 6: logs and final state."""
    loop = Loop(torch_cuda, sc)
    logs = loop.run(K6)
    return dict(logs=logs, final=loop.final())


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_cold_mode_is_the_cold_rollout(torch_cuda, sc, cold6):
    loop = WarmLoop(torch_cuda, sc)
    lg = loop.run_start(K6, COLD)
    fin = loop.final()
    used = lg.pop("start_used")
    same(lg, cold6["logs"], "logs")
    same({k: v for k, v in fin.items() if not k.startswith("carry_")}, cold6["final"], "state")
    assert (used == 0).all()
    assert loop.s.last_kernel.startswith("k_start_wide<")
    # the carry: the last tick's record, pose and flag
    N = loop.s.N
    run = running(fin["done"], K6 - 1)
    assert run.sum() > 40 and (~run).sum() >= 1  # (robots of the straight courses are done by tick 6)
    x = fin["carry_sol"][:, :8 * N - 2]
    np.testing.assert_array_equal(x[run][:, 6 * N], lg["cmd"][-1, run, 1])
    np.testing.assert_array_equal(x[run][:, 7 * N - 1], lg["cmd"][-1, run, 2])
    np.testing.assert_array_equal(fin["carry_ok"], (run & np.isin(lg["status"][-1], (1, 4))).astype(np.int32))
    np.testing.assert_array_equal(fin["carry_pose"][run], lg["pose"][-1, run])
    assert (fin["carry_sol"][fin["done"] > 0] == 0).all()  # (an invalid row's record: zeros)


@pytest.fixture(scope="module", params=[FULL], ids=["FULL"])
def warm(request, torch_cuda, sc):
    """One K = 6 call in the mode, and six K = 1 calls with the carry and the state snapshotted after
    each."""
    mode = request.param
    a = WarmLoop(torch_cuda, sc)
    la = a.run_start(K6, mode)
    fa = a.final()
    b = WarmLoop(torch_cuda, sc)
    ticks, snaps = [], [b.final()]
    for _ in range(K6):
        ticks.append(b.run_start(1, mode))
        snaps.append(b.final())
    return dict(mode=mode, logs=la, final=fa, ticks=ticks, snaps=snaps, P=a.P, sc=a.sc)


def test_one_call_equals_six_calls(warm):
    la, fa = warm["logs"], warm["final"]
    done = np.zeros(len(fa["done"]), dtype=np.int32)
    for k, lb in enumerate(warm["ticks"]):
        for name in la:
            assert la[name][k].tobytes() == lb[name][0].tobytes(), (name, k)
        d = warm["snaps"][k + 1]["done"]
        done[(done == 0) & (d == 1)] = k + 1
    fb = warm["snaps"][-1]
    for name in fa:
        if name != "done":
            assert fa[name].tobytes() == fb[name].tobytes(), name
    np.testing.assert_array_equal(fa["done"], done)


def test_tick_zero_is_the_cold_tick(warm, cold6):
    for name, v in cold6["logs"].items():
        assert warm["logs"][name][0].tobytes() == v[0].tobytes(), name
    assert (warm["logs"]["start_used"][0] == 0).all()


def test_start_used_and_done_robots(warm):
    lg, fin, mode = warm["logs"], warm["final"], warm["mode"]
    iters_warm = iters_n = 0
    for k in range(1, K6):
        run = running(fin["done"], k)
        ok = warm["snaps"][k]["carry_ok"] != 0
        assert (lg["start_used"][k][run & ok] == mode).all(), k
        assert (lg["start_used"][k][run & ~ok] == COLD).all(), k
        assert (lg["start_used"][k][~run] == 0).all() and (lg["status"][k][~run] == 13).all(), k
        assert (warm["snaps"][k + 1]["carry_ok"][~run] == 0).all(), k
        assert (run & ok).sum() > 40, k
        iters_warm += int(lg["iters"][k][run & ok].sum())
        iters_n += int((run & ok).sum())
    print(f"mode {mode}: {iters_warm / iters_n:.2f} iterations per started robot-tick")
    assert (fin["done"] > 0).sum() >= 1


def motion_on_device(torch, p0, p1):
    """The rollout's formula, one rounding per operation as the kernel evaluates it."""
    dX, dY = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1]
    c0, s0, dpsi = torch.cos(p0[:, 2]), torch.sin(p0[:, 2]), p1[:, 2] - p0[:, 2]
    return torch.stack([c0 * dX + s0 * dY, -s0 * dX + c0 * dY, torch.atan2(torch.sin(dpsi), torch.cos(dpsi))],
                       dim=1).contiguous()


def test_a_warm_tick_is_the_composition_of_the_device_calls(torch_cuda, warm):
    """Every tick k >= 1 and every robot running at it: the window, the preprocessing with the robot's
    count, the shift of its carried record and the started solve with its row, called one after the
    other on the logged inputs, give the logged u0, status and iterations bitwise and the speed to
    1e-15; the certificate of the records carried out of every tick is within the tolerances
    wherever the status is 1 or 4."""
    torch = torch_cuda
    from mpc_ros_amd import closed_loop, params, solver
    from mpc_ros_amd.solver import BatchSolver

    lg, fin, mode, P, scn = warm["logs"], warm["final"], warm["mode"], warm["P"], warm["sc"]
    B = len(fin["done"])
    N = int(P["STEPS"])
    from test_gpu_rollout import pack_courses

    packed, lens = pack_courses(scn["courses"])
    courses, tlens, course_of = dev(torch, packed), dev(torch, lens), dev(torch, scn["course_of"])
    mmax = closed_loop.plan_window_mmax(WINDOW_WP, STRIDE)
    s = BatchSolver(0, P)
    p = s.params
    compared, worst = 0, np.zeros(3)
    for k in range(1, K6):
        before = warm["snaps"][k]
        run = running(fin["done"], k)
        pose, vel = dev(torch, lg["pose"][k]), dev(torch, lg["vel"][k])
        cursor = dev(torch, before["cursor"])
        plan = torch.zeros((B, mmax, 2), dtype=torch.float64, device="cuda:0")
        count = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        s.plan_window_device(courses, tlens, course_of, pose, WINDOW_WP, STRIDE, cursor, plan, count)
        state = torch.zeros((B, 6), dtype=torch.float64, device="cuda:0")
        coeffs = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
        s.preprocess_device(pose, vel, plan, state, coeffs, delay_mode=True, count=count)
        rows = dev(torch, params.rows(P, REF_V=lg["ref_v"][k]))
        use = (before["carry_ok"] != 0) & run
        motion = motion_on_device(torch, dev(torch, before["carry_pose"]), pose)
        rec = dev(torch, before["carry_sol"])
        s.shift_solution_device(state, coeffs, motion, rec, rec, mask=dev(torch, use.astype(np.int32)), pparams=rows)
        u0 = torch.zeros((B, 2), dtype=torch.float64, device="cuda:0")
        status = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        iters = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        used = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        s.solve_device(state, coeffs, u0, status=status, iters=iters, pparams=rows, sol=rec, start=rec,
                       start_mode=dev(torch, np.where(use, mode, COLD).astype(np.int32)),
                       mu0=torch.full((B,), MU0, dtype=torch.float64, device="cuda:0"), start_used=used)
        torch.cuda.synchronize()
        gu, gs, gi = u0.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()
        assert gu[run].tobytes() == np.ascontiguousarray(lg["cmd"][k, run, 1:3]).tobytes(), k
        np.testing.assert_array_equal(gs[run], lg["status"][k, run])
        np.testing.assert_array_equal(gi[run], lg["iters"][k, run])
        np.testing.assert_array_equal(used.cpu().numpy()[run], lg["start_used"][k, run])
        speed = np.minimum(lg["vel"][k, :, 0] + gu[:, 1] * P["DT"], lg["ref_v"][k])
        assert np.abs(speed - lg["cmd"][k, :, 0])[run].max() <= 1e-15
        assert rec.cpu().numpy()[run].tobytes() == warm["snaps"][k + 1]["carry_sol"][run].tobytes(), k
        compared += int(run.sum())
        # the records carried out of this tick, on its problems
        cert = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
        s.kkt_device(state, coeffs, dev(torch, warm["snaps"][k + 1]["carry_sol"]), cert, pparams=rows)
        torch.cuda.synchronize()
        cert = cert.cpu().numpy()
        fine = run & np.isin(lg["status"][k], (1, 4))
        assert fine.sum() > 40
        worst = np.maximum(worst, cert[fine, :3].max(axis=0))
        assert cert[fine, 0].max() <= p.dual_inf_tol and cert[fine, 1].max() <= p.constr_viol_tol, k
        assert cert[fine, 2].max() <= p.compl_inf_tol, k
        np.testing.assert_array_equal(warm["snaps"][k + 1]["carry_ok"], fine.astype(np.int32))
    assert compared > 0.6 * (K6 - 1) * B
    print(f"mode {mode}: certificates of the carried records, dual {worst[0]:.2e} primal {worst[1]:.2e} compl "
          f"{worst[2]:.2e}")


def test_warm_real_robot_tick_leaves_the_pose_alone(torch_cuda, sc, warm):
    """integrate = 0: pose and feedback are the caller's, the command is the integrating tick's."""
    loop = WarmLoop(torch_cuda, sc)
    lg = loop.run_start(1, warm["mode"], integrate=False)
    fin = loop.final()
    np.testing.assert_array_equal(fin["pose"], sc["pose"])
    np.testing.assert_array_equal(fin["vel"], sc["vel"])
    for name in lg:
        assert lg[name][0].tobytes() == warm["logs"][name][0].tobytes(), name


def test_warm_rollout_in_a_captured_graph(torch_cuda, sc, warm):
    """K = 3 captured after one warm-up call on the capture stream, replayed twice from the restored
    inputs and a zeroed carry: logs, state and carry bitwise the direct call's."""
    torch = torch_cuda
    mode = warm["mode"]
    loop = WarmLoop(torch, sc)
    logs = loop.s.rollout_logs(3, loop.B)
    used = torch.zeros((3, loop.B), dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        loop.call_start(3, logs, used, mode, stream=side)  # (warm-up: the handle's buffers exist afterwards)
    torch.cuda.synchronize()
    direct = loop.final()
    want = {k: v[:3] for k, v in warm["logs"].items()}
    assert used.cpu().numpy().tobytes() == want["start_used"].tobytes()
    loop.restore()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        loop.call_start(3, logs, used, mode, stream=side)
    for _ in range(2):
        loop.restore()
        for t in list(logs.values()) + [used]:
            t.fill_(-7)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        for name, t in logs.items():
            assert t.cpu().numpy().tobytes() == want[name].tobytes(), name
        assert used.cpu().numpy().tobytes() == want["start_used"].tobytes()
        fin = loop.final()
        for name in fin:
            assert fin[name].tobytes() == direct[name].tobytes(), name


def test_warm_rollout_refusals(torch_cuda, sc):
    """A NULL carry pointer, PRIMAL or an unknown mode, a mu0 that is not positive and finite in FULL mode and
    the cold rollout's own refusals: refused before anything is queued, state and carry untouched."""
    torch = torch_cuda
    from mpc_ros_amd import _lib

    loop = WarmLoop(torch, sc)
    for t in loop.carry.values():
        t.fill_(3)
    before = loop.final()
    logs = loop.s.rollout_logs(1, loop.B)
    used = torch.zeros((1, loop.B), dtype=torch.int32, device="cuda:0")
    for kw in (dict(mode=3), dict(mode=-1), dict(mode=PRIMAL), dict(mode=FULL, mu0=0.0), dict(mode=FULL, mu0=-1.0),
               dict(mode=FULL, mu0=float("nan")), dict(mode=FULL, mu0=float("inf"))):
        with pytest.raises(_lib.MpcgError):
            loop.call_start(1, logs, used, **kw)
    with pytest.raises(_lib.MpcgError):
        loop.call_start(0, None, None, FULL)
    st = loop.state
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lgs = _lib.MpcgRolloutLogs()
    for missing in range(3):
        carry = [ptr(loop.carry[k]) for k in ("sol", "pose", "ok")]
        carry[missing] = None
        rc = _lib.lib().mpcg_rollout_device_start(
            loop.s._h, loop.B, 1, ptr(loop.courses), ptr(loop.lens), ptr(loop.course_of), loop.courses.shape[0],
            loop.courses.shape[1], WINDOW_WP, STRIDE, GOAL_TOL, VMAX, VMIN, 1, 1, ptr(st["pose"]), ptr(st["vel"]),
            ptr(st["cursor"]), ptr(st["ref_v"]), ptr(st["done"]), C.byref(lgs), None, FULL, MU0, *carry, None)
        assert rc == -1 and b"carry" in _lib.lib().mpcg_last_error()
    torch.cuda.synchronize()
    same(loop.final(), before, "state and carry")
    loop.call_start(1, logs, used, COLD, mu0=float("nan"))  # (mu0 is read in FULL mode only)
    torch.cuda.synchronize()
    assert C.sizeof(_lib.MpcgRolloutLogs) == 9 * C.sizeof(C.c_void_p)


# ------------------------------------------------------------------ 3. class MPC
def test_cpp_class_carries_its_solution(torch_cuda, tmp_path, infinity_golden):
    """tests/native/mpc_carry_check.cpp: three consecutive Solves in PRIMAL mode, carry_motion before
    the second only.  The second is the solve started from the first one's record shifted by
    mpcg_shift_solution, the third the solve started from the second one's record as it is (the
    motion is one-shot): both bitwise the Python calls'."""
    from mpc_ros_amd import solver
    from mpc_ros_amd.solver import BatchSolver

    exe = str(tmp_path / "mpc_carry")
    lib = os.path.join(ROOT, "mpc_ros_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "mpc_carry_check.cpp"), "-L", lib, "-lmpcg",
                           "-L/opt/rocm/lib", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    P = {"DT": 0.1, "STEPS": 20, "REF_CTE": 0.0, "REF_ETHETA": 0.0, "REF_V": 1.0, "W_CTE": 1000, "W_EPSI": 1000,
         "W_V": 100, "W_ANGVEL": 100, "W_A": 50, "W_DANGVEL": 0, "W_DA": 10, "ANGVEL": 1.0, "MAXTHR": 1.0,
         "BOUND": 1000}
    N = 20
    s = BatchSolver(0, P)
    g = infinity_golden
    st, cf = g["state"][:1].copy(), g["coeffs"][:1].copy()
    r0 = s.solve(st, cf, want_solution=True)
    assert r0["status"][0] == 1
    motion = np.array([[r0["x"][0, 1], r0["x"][0, N + 1], r0["x"][0, 2 * N + 1]]])
    chain, want = [(st, cf, np.zeros((1, 3)), 0)], [(COLD, r0)]
    st1, cf1 = st.copy(), cf.copy()
    st1[:, 3:6] += (0.02, 0.01, -0.01)
    cf1[:, 0] += 0.01
    start = solver.shift_solution(dict(P), st1, cf1, motion, r0["sol"])
    r1 = s.solve(st1, cf1, want_solution=True, start=start, start_mode=PRIMAL)
    chain.append((st1, cf1, motion, 1))
    want.append((PRIMAL, r1))
    st2, cf2 = st1.copy(), cf1.copy()
    st2[:, 3:6] += (0.02, 0.01, -0.01)
    r2 = s.solve(st2, cf2, want_solution=True, start=r1["sol"], start_mode=PRIMAL)
    chain.append((st2, cf2, motion, 0))
    want.append((PRIMAL, r2))
    assert r1["status"][0] in (1, 4) and r1["start_used"][0] == PRIMAL and r2["start_used"][0] == PRIMAL
    text = "\n".join(" ".join(repr(float(v)) for v in np.r_[a[0], b[0], m[0], f]) for a, b, m, f in chain) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, check=True).stdout.strip()
    lines = [ln.split() for ln in out.split("\n")]
    assert [ln[0] for ln in lines] == ["carry"] * 3 + ["sol"]
    for ln, (used, r) in zip(lines, want):
        assert int(ln[1]) == used and int(ln[2]) == r["iters"][0], ln[:3]
        assert np.array(ln[3:], dtype=np.float64).tobytes() == r["u0"][0].tobytes()
    sol = np.array(lines[3][2:], dtype=np.float64)
    assert int(lines[3][1]) == solver.solution_elems(N) and sol.tobytes() == r2["sol"][0].tobytes()
