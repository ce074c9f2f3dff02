"""A solution record carried to the next tick, on the host (no GPU needed).

mpcg_shift_solution (mpc_ros_amd/csrc/mpcg_shift.h, the code the kernel runs per lane) against
np_shift below, an independent numpy restatement of the rule's table in include/mpcg.h: the mapped
entries (x, y, theta of the moved stages, the terminal state, the (x, y) multiplier rows) to 1e-12
absolute, every entry that is only moved bit for bit.  Records: the cold solutions of fixture rows
at N = 3, 20, 65 and the bicycle's 25 (tests/test_start_host.py's shared cases), random finite
records at N = 2, 33, 128.

A shifted PRIMAL start against the oracle from the same shifted x, and a closed loop on the host
emulation (tests/native/wide_start_check.cpp) run five ways.  Iterations summed over the loop's 16
robots x 10 ticks, printed by test_closed_loop_five_ways (DESIGN.md "Carry to the next tick"):
cold 1656; PRIMAL unshifted 1446, shifted 1423; FULL (mu0 = 1e-4) unshifted 1266, shifted 1312.  The 32
shifted PRIMAL starts of the oracle test take 284 iterations, the same rows unshifted 261, cold 428.
"""
from __future__ import annotations

import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_solution_host import split
from test_start_host import (COLD, FULL, MU0, PRIMAL, SKIP_CAP, X_ATOL, case, neighbour, oracle_from, run_start,
                             shim)

MAP_ATOL = 1e-12


# ---------------------------------------------------------------- the rule, restated in numpy
def np_step(P, coeffs, s, u):
    """One step of FG_eval's model from stage values s[6] under controls u[2]."""
    dt = P["DT"]
    x, y, th, v, _, eth = s
    turn = v * u[0] / P["LF"] * dt if int(P.get("MODEL", 0)) == 1 else u[0] * dt
    fx = coeffs[0] + coeffs[1] * x + coeffs[2] * x ** 2 + coeffs[3] * x ** 3
    return np.array([x + v * math.cos(th) * dt, y + v * math.sin(th) * dt, th + turn, v + u[1] * dt,
                     (fx - y) + v * math.sin(eth) * dt, eth + turn])


def np_shift(P, state, coeffs, motion, rec):
    """The output record of one problem and the mask of its mapped entries."""
    N = int(P["STEPS"])
    nx = 8 * N - 2
    x, zl, zu, lam = (np.array(a) for a in split(rec, N))
    mx, my, mpsi = motion
    c, s = math.cos(mpsi), math.sin(mpsi)
    held = lambda a: np.concatenate([a[:, 1:], a[:, -1:]], axis=1)  # noqa: E731  (row k <- k + 1, the last held)
    X, U = x[:6 * N].reshape(6, N), x[6 * N:].reshape(2, N - 1)
    oX, oU = np.empty((6, N)), held(U)
    src = X[:, 1:]
    px, py = src[0] - mx, src[1] - my
    oX[0, :N - 1], oX[1, :N - 1], oX[2, :N - 1] = c * px + s * py, -s * px + c * py, src[2] - mpsi
    oX[3:, :N - 1] = src[3:]
    oX[:, 0] = state
    oX[:, N - 1] = np_step(P, coeffs, oX[:, N - 2], oU[:, N - 2])
    mX = np.zeros((6, N), dtype=bool)
    mX[:3, 1:N - 1] = True
    mX[:, N - 1] = True
    outs, masks = [np.r_[oX.ravel(), oU.ravel()]], [np.r_[mX.ravel(), np.zeros(2 * (N - 1), dtype=bool)]]
    for z in (zl, zu):
        outs.append(np.r_[held(z[:6 * N].reshape(6, N)).ravel(), held(z[6 * N:].reshape(2, N - 1)).ravel()])
        masks.append(np.zeros(nx, dtype=bool))
    L = held(lam.reshape(6, N))
    oL = L.copy()
    oL[0], oL[1] = c * L[0] + s * L[1], -s * L[0] + c * L[1]
    mL = np.zeros((6, N), dtype=bool)
    mL[:2] = True
    return np.concatenate(outs + [oL.ravel()]), np.concatenate(masks + [mL.ravel()])


# ---------------------------------------------------------------- the shapes
SHAPES = [(2, None), (3, "variants_N3"), (20, "infinity_N20"), (33, None), (65, "resto_N65"), (128, None),
          (25, "bicycle_N25")]


def motions(rng, B):
    """Small motions of a control period, then zero motion and headings near +-pi in the first rows."""
    m = np.stack([rng.uniform(-0.1, 0.1, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.3, 0.3, B)], axis=1)
    m[0] = 0.0
    m[1 % B] = (0.03, -0.01, math.pi - 1e-9)
    m[2 % B] = (-0.02, 0.04, -math.pi + 1e-9)
    m[3 % B] = (0.05, 0.02, math.pi)
    return m


_shapes = {}


def shape_case(N, name, oracle, tmp_path_factory):
    """(P, new state, new coeffs, motion, source records) of a shape, computed once."""
    if (N, name) not in _shapes:
        rng = np.random.default_rng(1000 + N)
        if name is None:
            from mpc_ros_amd import params

            B = 6
            P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
            state = rng.uniform(-0.5, 0.5, (B, 6))
            coeffs = rng.uniform(-0.3, 0.3, (B, 4))
            rec = rng.uniform(-3.0, 3.0, (B, 3 * (8 * N - 2) + 6 * N))
        else:
            r = case(name, oracle, tmp_path_factory)
            B = min(len(r["state"]), 16)
            P = dict(r["P"])
            state, coeffs = (a[:B] for a in neighbour(r["state"], r["coeffs"]))
            rec = np.array(r["cold"]["sol"][:B])
        assert int(P["STEPS"]) == N
        m = motions(rng, B)
        if name == "infinity_N20":  # (and each record's own motion to its stage 1: a loop's)
            m[4:] = np.stack([rec[4:, 1], rec[4:, N + 1], rec[4:, 2 * N + 1]], axis=1)
        _shapes[(N, name)] = (P, np.ascontiguousarray(state), np.ascontiguousarray(coeffs), m, rec)
    return _shapes[(N, name)]


@pytest.fixture(params=SHAPES, ids=lambda s: f"N{s[0]}_{s[1] or 'random'}")
def sh(request, oracle, tmp_path_factory, libmpcg):
    return shape_case(*request.param, oracle, tmp_path_factory)


def test_host_shift_equals_the_numpy_rule(sh):
    from mpc_ros_amd import solver

    P, state, coeffs, m, rec = sh
    assert np.isfinite(rec).all()
    got = solver.shift_solution(dict(P), state, coeffs, m, rec)
    worst = 0.0
    for b in range(len(state)):
        want, mapped = np_shift(P, state[b], coeffs[b], m[b], rec[b])
        d = np.abs(got[b] - want)
        worst = max(worst, d[mapped].max())
        assert d[mapped].max() <= MAP_ATOL, (b, d[mapped].max())
        assert got[b][~mapped].tobytes() == want[~mapped].tobytes(), b
    print(f"N = {P['STEPS']}: max |mapped - numpy| = {worst:.2e}, max |lambda| = "
          f"{np.abs(split(rec, int(P['STEPS']))[3]).max():.2e}")


def test_points_keep_their_place_in_the_world(sh):
    """The direction of the map: with the old pose p0 and the new pose p1 = p0 moved by `motion`,
    a point of the output seen from p1 is the source's point of the next stage seen from p0, and a
    heading likewise."""
    from mpc_ros_amd import solver

    P, state, coeffs, m, rec = sh
    N = int(P["STEPS"])
    got = solver.shift_solution(dict(P), state, coeffs, m, rec)
    if N < 3:
        # (N = 2 moves no stage: stage 0 is the new state, and the motion does not reach stage 1,
        # the model's step from it)
        far = solver.shift_solution(dict(P), state, coeffs, m + (0.5, -0.25, 1.0), rec)
        assert split(got, N)[0].tobytes() == split(far, N)[0].tobytes()
        assert split(got, N)[0][:, 0:6 * N:N].tobytes() == state.tobytes()
        return
    rng = np.random.default_rng(N)
    for b in range(len(state)):
        X0, Y0, psi0 = rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-math.pi, math.pi)
        mx, my, mpsi = m[b]
        X1 = X0 + math.cos(psi0) * mx - math.sin(psi0) * my
        Y1 = Y0 + math.sin(psi0) * mx + math.cos(psi0) * my
        psi1 = psi0 + mpsi
        world = lambda X, Y, psi, x, y: (X + math.cos(psi) * x - math.sin(psi) * y,  # noqa: E731
                                         Y + math.sin(psi) * x + math.cos(psi) * y)
        x, o = split(rec[b], N)[0], split(got[b], N)[0]
        wx0, wy0 = world(X0, Y0, psi0, x[2:N], x[N + 2:2 * N])
        wx1, wy1 = world(X1, Y1, psi1, o[1:N - 1], o[N + 1:2 * N - 1])
        assert np.abs(wx1 - wx0).max() <= MAP_ATOL and np.abs(wy1 - wy0).max() <= MAP_ATOL, b
        assert np.abs((o[2 * N + 1:3 * N - 1] + psi1) - (x[2 * N + 2:3 * N] + psi0)).max() <= MAP_ATOL, b


def test_last_step_has_no_defect_and_stage_zero_is_the_state(sh):
    from mpc_ros_amd import solver

    P, state, coeffs, m, rec = sh
    N = int(P["STEPS"])
    got = solver.shift_solution(dict(P), state, coeffs, m, rec)
    for b in range(len(state)):
        o = split(got[b], N)[0]
        X, U = o[:6 * N].reshape(6, N), o[6 * N:].reshape(2, N - 1)
        assert X[:, 0].tobytes() == state[b].tobytes()
        assert np.abs(X[:, N - 1] - np_step(P, coeffs[b], X[:, N - 2], U[:, N - 2])).max() <= MAP_ATOL, b


def test_mask_and_in_place(sh):
    from mpc_ros_amd import solver

    P, state, coeffs, m, rec = sh
    B = len(state)
    out = solver.shift_solution(dict(P), state, coeffs, m, rec)
    mask = (np.arange(B) % 3 != 1).astype(np.int32)
    part = solver.shift_solution(dict(P), state, coeffs, m, rec, mask=mask)
    keep = mask == 0
    assert keep.any() and (~keep).any()
    assert part[keep].tobytes() == rec[keep].tobytes() and part[~keep].tobytes() == out[~keep].tobytes()
    inplace = rec.copy()
    assert solver.shift_solution(dict(P), state, coeffs, m, inplace, out=inplace) is inplace
    assert inplace.tobytes() == out.tobytes()
    inplace = rec.copy()
    solver.shift_solution(dict(P), state, coeffs, m, inplace, mask=mask, out=inplace)
    assert inplace.tobytes() == part.tobytes()
    # a row per problem: the handle-less call's own parameters as rows give the same bits
    import ctypes as C

    from mpc_ros_amd import _lib

    p = solver._params_struct(dict(P), "fp64", {})
    rows = np.zeros((B, _lib.PP_FIELDS))
    _lib.check(_lib.lib().mpcg_pparams_fill(C.byref(p), B, rows.ctypes.data_as(C.POINTER(C.c_double))), "fill")
    assert solver.shift_solution(p, state, coeffs, m, rec, params_rows=rows).tobytes() == out.tobytes()
    rows[:, 0] *= 2.0  # (DT: the terminal step moves)
    assert solver.shift_solution(p, state, coeffs, m, rec, params_rows=rows).tobytes() != out.tobytes()


def test_non_finite_entries_pass_through(libmpcg, oracle, tmp_path_factory):
    from mpc_ros_amd import solver

    P, state, coeffs, m, rec = shape_case(33, None, oracle, tmp_path_factory)
    N, bad = 33, rec.copy()
    nx = 8 * N - 2
    bad[0, 4 * N + 5] = np.nan       # cte of stage 5 -> stage 4
    bad[1, nx + 6 * N + 3] = np.inf  # zl of control 3 -> control 2
    got = solver.shift_solution(dict(P), state, coeffs, m, bad)
    assert np.isnan(got[0, 4 * N + 4]) and np.isinf(got[1, nx + 6 * N + 2])
    assert np.isfinite(got[2:]).all()


def test_refusals(libmpcg):
    import ctypes as C

    L = libmpcg
    from mpc_ros_amd import _lib

    p = _lib.MpcgParams()
    L.mpcg_params_plugin_default(C.byref(p))
    one = (C.c_double * 600)()
    dp = C.cast(one, C.POINTER(C.c_double))
    assert L.mpcg_shift_solution(None, 1, dp, dp, None, dp, None, dp, dp) == -1
    assert L.mpcg_shift_solution(C.byref(p), -1, dp, dp, None, dp, None, dp, dp) == -1
    assert L.mpcg_shift_solution(C.byref(p), 1, dp, dp, None, None, None, dp, dp) == -1
    assert b"motion" in L.mpcg_last_error()
    assert L.mpcg_shift_solution(C.byref(p), 0, None, None, None, None, None, None, None) == 0
    assert L.mpcg_shift_solution_device(None, 1, *([None] * 8)) == -1
    assert b"null handle" in L.mpcg_last_error()
    assert L.mpcg_rollout_device_start(None, 1, 1, *([None] * 3), 1, 1, 1, 1, 0.1, 0.7, 0.05, 1, 1, *([None] * 7), 1, 1e-4,
                                       None, None, None, None) == -1
    assert L.mpcg_abi_version() == 2


def test_stage_rule_under_sanitizers(tmp_path):
    """tests/native/shift_check.cpp: a stand-alone program over mpcg_shift.h, built with ASan and
    UBSan and run directly."""
    exe = str(tmp_path / "shift_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'mpc_ros_amd', 'csrc')}", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "shift_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr


# ---------------------------------------------------------------- a shifted PRIMAL start against the oracle
def test_shifted_primal_start_equals_the_oracle(oracle, tmp_path_factory, libmpcg):
    """32 infinity rows: the cold record of row b, shifted by its own motion to stage 1 (the pose the
    solution predicts one control period on), starts the neighbour problem of row b
    (test_start_host.neighbour) in PRIMAL mode on the host emulation; the oracle is solved from the
    same shifted x.  The same status and iteration count, x within 1e-7.  A row is left out only
    where the oracle's own count differs between kkt_structured 0 and 1 for that start, at most 1
    row in 32 (test_start_host.SKIP_CAP's ratio)."""
    from mpc_ros_amd import solver

    r = case("infinity_N20", oracle, tmp_path_factory)
    N, P, o = r["N"], r["P"], r["opts"]
    rows = slice(0, 32)
    state, coeffs = r["nstate"][rows], r["ncoeffs"][rows]
    rec = np.array(r["cold"]["sol"][rows])
    motion = np.stack([rec[:, 1], rec[:, N + 1], rec[:, 2 * N + 1]], axis=1)
    start = solver.shift_solution(dict(P), state, coeffs, motion, rec)
    x0 = np.ascontiguousarray(split(start, N)[0])
    got = run_start(r["exe"], P, state, coeffs, o, PRIMAL, start)
    L = shim(oracle, tmp_path_factory)
    st0, it0, xs0 = oracle_from(oracle, L, P, o, state, coeffs, x0, 0)
    _, it1, _ = oracle_from(oracle, L, P, o, state, coeffs, x0, 1)
    moves = it0 != it1
    keep = ~moves
    d = np.abs(split(got["sol"], N)[0] - xs0).max(axis=1)
    unshifted = run_start(r["exe"], P, state, coeffs, o, PRIMAL, rec)
    print(f"shifted PRIMAL: left out {np.flatnonzero(moves)}; max |x - oracle x| = {d[keep].max():.3e}; iterations "
          f"{got['iters'].sum()} (unshifted {unshifted['iters'].sum()}, cold {r['ncold']['iters'][rows].sum()})")
    assert moves.sum() <= SKIP_CAP["infinity_N20"] // 2  # (1 in 32: SKIP_CAP's 2 in 64)
    assert (got["used"] == PRIMAL).all()
    np.testing.assert_array_equal(got["status"][keep], st0[keep])
    np.testing.assert_array_equal(got["iters"][keep], it0[keep])
    assert d[keep].max() <= X_ATOL


# ---------------------------------------------------------------- a closed loop, five ways
WAYS = [("cold", COLD, False), ("PRIMAL unshifted", PRIMAL, False), ("PRIMAL shifted", PRIMAL, True),
        ("FULL unshifted", FULL, False), ("FULL shifted", FULL, True)]
B_LOOP, TICKS = 16, 10


def test_closed_loop_five_ways(oracle, tmp_path_factory, libmpcg):
    """16 robots on the lemniscate, 10 ticks, on the host emulation.  The loop is closed with the
    cold solve's commands (closed_loop.run's unicycle and plan, the oracle's preprocessing), so all
    five ways solve the same problem at every tick; each way starts a tick from its own record of
    the tick before -- as it is, or shifted by the robots' motion between the two poses (the
    rollout's formula) -- wherever that record is a solution (status 1 or 4), else cold.  Every
    started tick ends with status 1 or 4 wherever the cold one does, within the three tolerances of
    the certificate (mpcg_kkt).  The five iteration sums are printed (the module docstring)."""
    from mpc_ros_amd import closed_loop, infinity, solver
    from test_solution_host import fixture_set

    from host_harness import build

    P, _ = fixture_set("infinity")
    N, dt = int(P["STEPS"]), P["DT"]
    o = oracle.ref_opts(N)
    exe = build("wide_start_check")
    ne = 3 * (8 * N - 2) + 6 * N
    arc = infinity._arc()
    t = 0.3 + 0.37 * np.arange(B_LOOP)
    hd = np.array([float(arc.heading(v)) for v in t])
    lat, herr = 0.15 * np.cos(1.0 * np.arange(B_LOOP)), 0.2 * np.sin(1.3 * np.arange(B_LOOP))
    px, py = arc.point(t)
    x, y, yaw = px - np.sin(hd) * lat, py + np.cos(hd) * lat, hd + herr
    vel = np.zeros((B_LOOP, 3))
    rec = {w[0]: np.zeros((B_LOOP, ne)) for w in WAYS}
    ok = {w[0]: np.zeros(B_LOOP, dtype=bool) for w in WAYS}
    sums = {w[0]: 0 for w in WAYS}
    started = {w[0]: 0 for w in WAYS}
    prev_pose = None
    for k in range(TICKS):
        pose = np.stack([x, y, np.arctan2(np.sin(yaw), np.cos(yaw))], axis=1)
        state, coeffs = np.zeros((B_LOOP, 6)), np.zeros((B_LOOP, 4))
        for b in range(B_LOOP):
            t[b] = closed_loop.nearest_t(x[b], y[b], t[b])
            rc, state[b], coeffs[b] = oracle.find_best_path(*pose[b], *vel[b], dt, closed_loop.plan_from(t[b]), True)
            assert rc == 0
        if prev_pose is not None:
            dX, dY = pose[:, 0] - prev_pose[:, 0], pose[:, 1] - prev_pose[:, 1]
            c0, s0, dpsi = np.cos(prev_pose[:, 2]), np.sin(prev_pose[:, 2]), pose[:, 2] - prev_pose[:, 2]
            motion = np.stack([c0 * dX + s0 * dY, -s0 * dX + c0 * dY, np.arctan2(np.sin(dpsi), np.cos(dpsi))], axis=1)
        res = {}
        for name, mode, shifted in WAYS:
            modes = np.where(ok[name], mode, COLD).astype(np.int32)
            start = rec[name]
            if shifted and prev_pose is not None:
                start = solver.shift_solution(dict(P), state, coeffs, motion, start, mask=ok[name].astype(np.int32))
            res[name] = g = run_start(exe, P, state, coeffs, o, modes, start, mu0=MU0)
            np.testing.assert_array_equal(g["used"], modes, err_msg=f"{name}, tick {k}")
            sums[name] += int(g["iters"].sum())
            started[name] += int((modes != COLD).sum())
            rec[name], ok[name] = g["sol"], np.isin(g["status"], (1, 4))
        cold = res["cold"]
        good = np.isin(cold["status"], (1, 4))
        assert good.mean() > 0.9, k
        for name, _, _ in WAYS[1:]:
            g = res[name]
            assert np.isin(g["status"][good], (1, 4)).all(), (name, k, g["status"], cold["status"])
            cert = solver.kkt(dict(P), state, coeffs, g["sol"])
            fine = np.isin(g["status"], (1, 4))
            assert cert[fine, 0].max() <= o.dual_inf_tol and cert[fine, 1].max() <= o.constr_viol_tol, (name, k)
            assert cert[fine, 2].max() <= o.compl_inf_tol, (name, k)
        # the cold loop's command closes the loop (driving_state.cpp:262-269, closed_loop.run)
        speed = np.minimum(vel[:, 0] + cold["u0"][:, 1] * dt, P["REF_V"])
        prev_pose = pose
        x, y, yaw = x + speed * np.cos(yaw) * dt, y + speed * np.sin(yaw) * dt, yaw + cold["u0"][:, 0] * dt
        vel = np.stack([speed, cold["u0"][:, 0], cold["u0"][:, 1]], axis=1)
    print("iterations over 16 robots x 10 ticks: " + "; ".join(f"{n} {sums[n]}" for n, _, _ in WAYS))
    for name, mode, _ in WAYS[1:]:
        assert started[name] >= 0.9 * B_LOOP * (TICKS - 1), name
