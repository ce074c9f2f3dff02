"""GPU: start point in (mpcg_solve_start / mpcg_solve_device_start; the k_start_wide and
k_resume_wide<START_RESUME> instances) against the host emulation of the same solver started the same way
(tests/native/wide_start_check.cpp, tests/test_start_host.py).

The problems are the neighbour problems of tests/test_start_host.py's shapes, each started from the
cold solution of its own row, the modes COLD / PRIMAL / FULL mixed per row in one batch.  x to 1e-7;
lambda and z to one relative tolerance, test_gpu_solution.py's: max(|d lambda|_inf, |d z|_inf) /
max(|lambda|_inf, |z|_inf) per row.  START_MULT_REL_MEASURED is the largest such difference measured
on an MI355X against the host emulation over all shapes (test_device_equals_the_host_emulation
prints every shape's); the tests allow ten times it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import solver_for, torch_cuda  # noqa: F401
from test_gpu_solution import X_ATOL, against_host, dev, gpu_solve, self_consistent
from test_start_host import (COLD, FULL, MU0, PRIMAL, RESTORING, SHAPES, U0_DIFF_BOUND, case, cold_point,
                             restoring_starts, run_start)

pytestmark = pytest.mark.gpu

START_MULT_REL_MEASURED = 2.295e-15
START_MULT_REL_BOUND = 10 * START_MULT_REL_MEASURED
OUT = ("u0", "traj", "status", "iters", "obj", "diag", "sol", "used")


def gpu_start(torch, s, st, cf, start, modes, mu0=MU0, rows=None, in_place=False, want_sol=True):
    """solve_device(start=...); the outputs as numpy arrays.  in_place: sol is the start tensor."""
    from mpc_ros_amd.solver import solution_elems

    B, N = st.shape[0], s.N
    d = torch.device("cuda:0")
    out = dict(u0=torch.full((B, 2), 7.0, dtype=torch.float64, device=d),
               traj=torch.full((B, 3, N), 7.0, dtype=torch.float64, device=d),
               status=torch.full((B,), -1, dtype=torch.int32, device=d),
               obj=torch.full((B,), 7.0, dtype=torch.float64, device=d),
               iters=torch.full((B,), -1, dtype=torch.int32, device=d),
               diag=torch.full((B, 4), -1, dtype=torch.int32, device=d))
    tstart = dev(torch, start)
    used = torch.full((B,), -9, dtype=torch.int32, device=d)
    sol = None
    if want_sol:
        sol = tstart if in_place else torch.full((B, solution_elems(N)), 7.0, dtype=torch.float64, device=d)
    tmode = dev(torch, np.ascontiguousarray(np.broadcast_to(np.asarray(modes, dtype=np.int32), (B,))))
    tmu = None if mu0 is None else dev(torch, np.ascontiguousarray(np.broadcast_to(np.float64(mu0), (B,))))
    s.solve_device(dev(torch, st), dev(torch, cf), pparams=None if rows is None else dev(torch, rows), sol=sol,
                   start=tstart, start_mode=tmode, mu0=tmu, start_used=used, **out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["used"] = used.cpu().numpy()
    if want_sol:
        r["sol"] = sol.cpu().numpy()
    return r


def mixed_modes(B):
    return (np.arange(B) % 3).astype(np.int32)


_host = {}


def host_mixed(name, oracle, tmp_path_factory):
    """The host emulation of a shape's neighbour problems in mixed modes, computed once."""
    if name not in _host:
        r = case(name, oracle, tmp_path_factory)
        modes = mixed_modes(len(r["nstate"]))
        h = run_start(r["exe"], r["P"], r["nstate"], r["ncoeffs"], r["opts"], modes, r["cold"]["sol"], mu0=MU0)
        for v in h.values():
            v.setflags(write=False)
        _host[name] = (r, modes, h)
    return _host[name]


# ------------------------------------------------------------------ 1, 2. against the host; COLD rows
@pytest.mark.parametrize("name", SHAPES)
def test_device_equals_the_host_emulation(torch_cuda, oracle, tmp_path_factory, name):  # noqa: F811
    r, modes, h = host_mixed(name, oracle, tmp_path_factory)
    N = r["N"]
    s = solver_for(r["P"])
    g = gpu_start(torch_cuda, s, r["nstate"], r["ncoeffs"], r["cold"]["sol"], modes)
    assert s.last_kernel.startswith("k_start_wide<")
    np.testing.assert_array_equal(g["used"], h["used"])
    np.testing.assert_array_equal(g["used"], modes)
    self_consistent(g, N)
    d = against_host(g, h, N)
    print(f"{name}: multipliers rel {d:.3e} over {len(modes)} rows; iterations {g['iters'].sum()}")
    assert d <= START_MULT_REL_BOUND
    # the COLD rows: bitwise the cold solve's outputs
    c = gpu_solve(torch_cuda, s, r["nstate"], r["ncoeffs"])
    cold = modes == COLD
    for k in ("u0", "traj", "status", "iters", "obj", "diag", "sol"):
        np.testing.assert_array_equal(g[k][cold], c[k][cold], err_msg=k)


def test_an_all_cold_batch_is_the_cold_solve(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    for name in ("infinity_N20", "resto_N20"):
        r = case(name, oracle, tmp_path_factory)
        s = solver_for(r["P"])
        c = gpu_solve(torch_cuda, s, r["state"], r["coeffs"])
        assert s.last_kernel.startswith("k_solve_wide<")
        junk = np.full_like(r["cold"]["sol"], np.nan)  # (not read)
        g = gpu_start(torch_cuda, s, r["state"], r["coeffs"], junk, COLD, mu0=None)
        assert (g["used"] == COLD).all()
        for k in ("u0", "traj", "status", "iters", "obj", "diag", "sol"):
            np.testing.assert_array_equal(g[k], c[k], err_msg=k)


# ------------------------------------------------------------------ 3. parked and overflow paths
def test_restoration_rows_do_not_depend_on_the_park_capacity(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    r = case("resto_N20", oracle, tmp_path_factory)
    st, cf = r["state"], r["coeffs"]
    start = cold_point(st, r["N"])
    h = run_start(r["exe"], r["P"], st, cf, r["opts"], PRIMAL, start)
    got = []
    for cap in (0, 1):
        s = solver_for(r["P"])
        s.set_park_capacity(cap)
        g = gpu_start(torch_cuda, s, st, cf, start, PRIMAL)
        assert (g["used"] == PRIMAL).all() and (g["diag"][:, 0] > 0).all()
        d2 = g["diag"][:, 2]
        assert (d2 == 1).all() if cap == 0 else ((d2 == 2).sum() >= len(d2) - 1 and (d2 >= 1).all())
        d = against_host(g, h, r["N"])
        print(f"resto_N20 from the cold point, park {cap}: multipliers rel {d:.3e}")
        assert d <= START_MULT_REL_BOUND
        got.append(g)
    for k in ("u0", "traj", "status", "iters", "obj", "sol", "used"):
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    np.testing.assert_array_equal(got[0]["diag"][:, [0, 1, 3]], got[1]["diag"][:, [0, 1, 3]])


def test_started_solves_through_the_parked_and_overflow_paths(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    """Starts that are not the cold point and restore (test_start_host.restoring_starts, tiled twice:
    four restoring problems among sixteen).  With the default park area all four are continued by
    k_resume_wide<START_RESUME> from their park entries (diag[:, 2] 1), with one park entry at least three
    are started again from their records by its overflow branch (2).  Either way the host emulation's
    iterates: a cold restart of the FULL rows would take 80 iterations instead of 70, and a PRIMAL
    row continued with the cold objective scale would report multipliers 1 % off."""
    r = case("resto_N20", oracle, tmp_path_factory)
    st, cf, modes, starts = restoring_starts(r)
    h = run_start(r["exe"], r["P"], st, cf, r["opts"], modes, starts, mu0=MU0)
    idx = np.r_[np.arange(8), np.arange(8)]
    hh = {k: v[idx] for k, v in h.items()}
    rest = np.isin(idx, RESTORING)
    got = []
    for cap in (0, 1):
        s = solver_for(r["P"])
        s.set_park_capacity(cap)
        g = gpu_start(torch_cuda, s, st[idx], cf[idx], starts[idx], modes[idx])
        np.testing.assert_array_equal(g["used"], modes[idx])
        np.testing.assert_array_equal(g["diag"][:, 0] > 0, rest)
        d2 = g["diag"][:, 2]
        assert (d2[~rest] == 0).all()
        if cap == 0:
            assert (d2[rest] == 1).all()
        else:
            assert (d2[rest] >= 1).all() and (d2[rest] == 2).sum() >= 3
        d = against_host(g, hh, r["N"])
        print(f"started and restoring, park {cap}: diag[:, 2] {d2[rest]}, multipliers rel {d:.3e}")
        assert d <= START_MULT_REL_BOUND
        got.append(g)
    for k in ("u0", "traj", "status", "iters", "obj", "sol", "used"):
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    assert (got[0]["iters"][rest] != np.r_[r["cold"]["iters"], r["cold"]["iters"], r["cold"]["iters"],
                                          r["cold"]["iters"]][rest]).all()


# ------------------------------------------------------------------ 4. in place
@pytest.mark.parametrize("name,cap", [("infinity_N20", 0), ("resto_N20", 1)])
def test_sol_may_alias_start(torch_cuda, oracle, tmp_path_factory, name, cap):  # noqa: F811
    """resto_N20 from the cold point with one park entry: the overflow re-solve reads the start
    again, after the other problems have written their records."""
    r = case(name, oracle, tmp_path_factory)
    s = solver_for(r["P"])
    s.set_park_capacity(cap)
    if name == "resto_N20":
        st, cf, start, modes = r["state"], r["coeffs"], cold_point(r["state"], r["N"]), PRIMAL
    else:
        st, cf, start, modes = r["nstate"], r["ncoeffs"], r["cold"]["sol"], mixed_modes(len(r["nstate"]))
    a = gpu_start(torch_cuda, s, st, cf, start, modes)
    b = gpu_start(torch_cuda, s, st, cf, start, modes, in_place=True)
    for k in OUT:
        assert a[k].tobytes() == b[k].tobytes(), k
    if cap:
        assert (a["diag"][:, 2] == 2).any()


# ------------------------------------------------------------------ 5. an ordered batch
def test_start_row_is_the_problems_own_in_an_ordered_batch(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    r, modes, _ = host_mixed("infinity_N20", oracle, tmp_path_factory)
    n = len(modes)
    idx = np.arange(2112) % n
    s = solver_for(r["P"])
    small = gpu_start(torch_cuda, s, r["nstate"], r["ncoeffs"], r["cold"]["sol"], modes)
    # (a start that belongs to another row would change the row's iterates: every third row FULL)
    big = gpu_start(torch_cuda, s, r["nstate"][idx], r["ncoeffs"][idx], r["cold"]["sol"][idx], modes[idx])
    assert s.last_solve_order
    for k in OUT:
        np.testing.assert_array_equal(big[k], small[k][idx], err_msg=k)


# ------------------------------------------------------------------ 6. rows
def test_a_started_solve_under_each_parameter_row(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    from mpc_ros_amd import params

    r = case("infinity_N20", oracle, tmp_path_factory)
    P, o, N = r["P"], r["opts"], r["N"]
    P2 = dict(P, REF_V=0.7 * P["REF_V"], W_CTE=2.0 * P["W_CTE"], ANGVEL=0.5 * P["ANGVEL"])
    rows = params.rows([P, P2, P2, P])
    modes = np.array([FULL, PRIMAL, FULL, PRIMAL], dtype=np.int32)
    st, cf = r["nstate"][:4], r["ncoeffs"][:4]
    starts, host = [], []
    for b, Pb in enumerate((P, P2, P2, P)):
        zero = np.zeros((1, r["cold"]["sol"].shape[1]))
        c = run_start(r["exe"], Pb, r["state"][b:b + 1], r["coeffs"][b:b + 1], o, COLD, zero)
        starts.append(c["sol"][0])
        host.append(run_start(r["exe"], Pb, st[b:b + 1], cf[b:b + 1], o, modes[b:b + 1], c["sol"], mu0=MU0))
    g = gpu_start(torch_cuda, solver_for(dict(P, REF_V=0.1, W_V=7.0)), st, cf, np.array(starts), modes, rows=rows)
    np.testing.assert_array_equal(g["used"], modes)
    for b in range(4):
        gb = {k: v[b:b + 1] for k, v in g.items()}
        self_consistent(gb, N)
        d = against_host(gb, host[b], N)
        print(f"row {b}: multipliers rel {d:.3e}")
        assert d <= START_MULT_REL_BOUND
    assert not np.array_equal(g["u0"][0], g["u0"][1])


# ------------------------------------------------------------------ 7. graph capture
def test_graph_capture_and_replay(torch_cuda, infinity_golden):  # noqa: F811
    from conftest import params_from_array
    from mpc_ros_amd.solver import solution_elems
    from test_start_host import neighbour

    torch = torch_cuda
    gi = infinity_golden
    P = params_from_array(gi["params"])
    B, N = 96, 20
    st0, cf0 = np.ascontiguousarray(gi["state"][:B]), np.ascontiguousarray(gi["coeffs"][:B])
    s = solver_for(P)
    s.reserve(B)
    start = gpu_solve(torch, s, st0, cf0)["sol"]
    st, cf = neighbour(st0, cf0)
    modes = mixed_modes(B)
    want = gpu_start(torch, s, st, cf, start, modes)
    d = torch.device("cuda:0")
    tst, tcf, tstart, tmode = dev(torch, st), dev(torch, cf), dev(torch, start), dev(torch, modes)
    tmu = torch.full((B,), MU0, dtype=torch.float64, device=d)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=d)
    status = torch.empty(B, dtype=torch.int32, device=d)
    iters = torch.empty(B, dtype=torch.int32, device=d)
    used = torch.empty(B, dtype=torch.int32, device=d)
    sol = torch.empty((B, solution_elems(N)), dtype=torch.float64, device=d)
    args = dict(status=status, iters=iters, sol=sol, start=tstart, start_mode=tmode, mu0=tmu, start_used=used)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        s.solve_device(tst, tcf, u0, **args)  # (warm-up on the capture stream)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        s.solve_device(tst, tcf, u0, **args)
    for _ in range(2):
        for t in (u0, sol):
            t.zero_()
        for t in (status, iters, used):
            t.fill_(-5)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        for k, t in (("u0", u0), ("status", status), ("iters", iters), ("used", used), ("sol", sol)):
            assert t.cpu().numpy().tobytes() == want[k].tobytes(), k


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    torch = torch_cuda
    from mpc_ros_amd import _lib

    r = case("variants_N3", oracle, tmp_path_factory)
    st, cf = dev(torch, r["nstate"]), dev(torch, r["ncoeffs"])
    B = len(r["nstate"])
    u0 = torch.zeros((B, 2), dtype=torch.float64, device="cuda:0")
    start = dev(torch, r["cold"]["sol"])
    mode = torch.full((B,), FULL, dtype=torch.int32, device="cuda:0")
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = solver_for(r["P"])
    none = [None] * 8
    rc = L.mpcg_solve_device_start(s._h, B, p(st), p(cf), None, None, p(mode), None, p(u0), *none)
    assert rc == -1 and b"start" in L.mpcg_last_error()
    rc = L.mpcg_solve_device_start(s._h, B, p(st), p(cf), None, p(start), None, None, p(u0), *none)
    assert rc == -1 and b"start_mode" in L.mpcg_last_error()
    s32 = solver_for(dict(r["P"], STEPS=20), dtype="fp32")
    with pytest.raises(_lib.MpcgError, match="precision 1"):
        s32.solve(r["nstate"], r["ncoeffs"], start=np.zeros((B, 3 * 158 + 120)), start_mode=COLD)
    assert (u0 == 0).all()
    g = gpu_start(torch, s, r["nstate"], r["ncoeffs"], r["cold"]["sol"], FULL)
    assert (g["used"] == FULL).all() and (g["status"] == 1).all()
    # the host-buffer call: the device call's bytes
    h = s.solve(r["nstate"], r["ncoeffs"], want_solution=True, start=r["cold"]["sol"], start_mode=FULL, mu0=MU0)
    for k in ("u0", "status", "iters", "obj", "sol"):
        np.testing.assert_array_equal(h[k], g[k], err_msg=k)
    np.testing.assert_array_equal(h["start_used"], g["used"])


def test_host_entries_return_their_device_twins_bytes(torch_cuda, infinity_golden):  # noqa: F811
    """Each host-pointer entry -- mpcg_solve_ex, _pp, _sol and _start, staged through the handle's io
    block (wide_plan.h IoLayout) -- returns byte for byte what its device-pointer twin returns, for
    every output, with rows, records, mu0, diag and start_used all given.  B is odd, so the int32
    regions of the block end off an 8-byte boundary."""
    from conftest import params_from_array
    from mpc_ros_amd import params

    torch = torch_cuda
    gi = infinity_golden
    P = params_from_array(gi["params"])
    B = 3
    st, cf = np.ascontiguousarray(gi["state"][:B]), np.ascontiguousarray(gi["coeffs"][:B])
    rows = params.rows([P, dict(P, REF_V=0.7 * P["REF_V"], W_CTE=2.0 * P["W_CTE"], ANGVEL=0.5 * P["ANGVEL"]), P])
    s = solver_for(P)
    assert s.N == 20
    outs = ("u0", "traj", "status", "obj", "iters", "diag")

    def same(h, g, keys):
        for k in keys:
            assert h[k].dtype == g[k].dtype and h[k].tobytes() == g[k].tobytes(), k

    same(s.solve(st, cf), gpu_solve(torch, s, st, cf, want_sol=False), outs)
    assert s.last_kernel.startswith("k_solve_wide<")
    same(s.solve(st, cf, params_rows=rows), gpu_solve(torch, s, st, cf, rows=rows, want_sol=False), outs)
    assert s.last_kernel.startswith("k_solve_wide_pp<")
    g = gpu_solve(torch, s, st, cf, rows=rows)
    same(s.solve(st, cf, params_rows=rows, want_solution=True), g, outs + ("sol",))
    modes = mixed_modes(B)
    gs = gpu_start(torch, s, st, cf, g["sol"], modes, mu0=MU0, rows=rows)
    hs = s.solve(st, cf, params_rows=rows, want_solution=True, start=g["sol"], start_mode=modes, mu0=MU0)
    assert s.last_kernel.startswith("k_start_wide<")
    same(hs, gs, outs + ("sol",))
    same({"used": hs["start_used"]}, gs, ("used",))
    assert not np.array_equal(gs["iters"], g["iters"])  # (the start was read)


# ------------------------------------------------------------------ 9. class MPC
def test_cpp_class_starts_from_its_last_solution(torch_cuda, tmp_path, infinity_golden):  # noqa: F811
    """tests/native/mpc_start_check.cpp: three consecutive Solves on a neighbour chain."""
    exe = str(tmp_path / "mpc_start")
    lib = os.path.join(ROOT, "mpc_ros_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "mpc_start_check.cpp"), "-L", lib, "-lmpcg",
                           "-L/opt/rocm/lib", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    g = infinity_golden
    st, cf = g["state"][0].copy(), g["coeffs"][0].copy()
    lines = []
    for _ in range(3):
        lines.append(" ".join(repr(float(v)) for v in np.r_[st, cf]))
        st[3:6] += (0.02, 0.01, -0.01)
        cf[0] += 0.01
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         check=True).stdout.strip().split("\n")
    cold = [ln.split() for ln in out[:3]]
    warm = [ln.split() for ln in out[3:]]
    assert all(c[0] == "cold" for c in cold) and all(w[0] == "start" for w in warm)
    assert [int(w[1]) for w in warm] == [COLD, FULL, FULL]
    print("iterations cold", [int(c[1]) for c in cold], "started", [int(w[2]) for w in warm])
    assert int(warm[0][2]) == int(cold[0][1])
    for c, w in zip(cold[1:], warm[1:]):
        assert int(w[2]) < int(c[1])
    for c, w in zip(cold, warm):
        du = np.abs(np.array(w[3:], dtype=float) - np.array(c[2:], dtype=float)).max()
        assert du <= U0_DIFF_BOUND
