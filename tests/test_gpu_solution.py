"""GPU: the full solution record (mpcg_solve_sol / mpcg_solve_device_sol; WideSolver::solution_out
called by every ending's write_out) against the record the host emulation of the same solver
writes (tests/native/wide_sol_check.cpp).

x to 1e-7, the project's control tolerance.  lambda and z to one relative tolerance.  They are
the unknowns of one linear system -- stationarity, grad f + J^T lambda - z_L + z_U = 0, with
coefficients of order one -- so a difference in either is measured against the same scale, the
row's largest multiplier: max(|d lambda|_inf, |d z|_inf) / max(|lambda|_inf, |z|_inf).  Host and
GPU run the same operations but contract other multiply-adds, so their iterates agree to rounding
only.  MULT_REL_MEASURED is the largest such difference measured on the infinity rows (N = 20;
test_record_equals_the_host_emulations prints every shape's), the tests allow ten times it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import params_from_array
from host_harness import build
from test_gpu_parity import solver_for, torch_cuda  # noqa: F401
from test_solution_host import fixture_set, run_sol_harness, split

pytestmark = pytest.mark.gpu

X_ATOL = 1e-7
# max over the 288 infinity rows of the difference above, measured on an MI355X against the host
# emulation
MULT_REL_MEASURED = 1.915e-15
MULT_REL_BOUND = 10 * MULT_REL_MEASURED
OUT = ("u0", "traj", "status", "iters", "obj")


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # (a copy: fixture arrays are read-only)


def gpu_solve(torch, s, st, cf, rows=None, want_sol=True):
    """solve_device (with the record unless want_sol is False); the outputs as numpy arrays."""
    from mpc_ros_amd.solver import solution_elems

    B, N = st.shape[0], s.N
    d = torch.device("cuda:0")
    out = dict(u0=torch.full((B, 2), 7.0, dtype=torch.float64, device=d),
               traj=torch.full((B, 3, N), 7.0, dtype=torch.float64, device=d),
               status=torch.full((B,), -1, dtype=torch.int32, device=d),
               obj=torch.full((B,), 7.0, dtype=torch.float64, device=d),
               iters=torch.full((B,), -1, dtype=torch.int32, device=d),
               diag=torch.full((B, 4), -1, dtype=torch.int32, device=d))
    if want_sol:
        out["sol"] = torch.full((B, solution_elems(N)), 7.0, dtype=torch.float64, device=d)
    s.solve_device(dev(torch, st), dev(torch, cf), pparams=None if rows is None else dev(torch, rows), **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def self_consistent(r, N):
    """x is bitwise the point u0 and traj publish."""
    x = split(r["sol"], N)[0]
    np.testing.assert_array_equal(x[:, :3 * N].reshape(-1, 3, N), r["traj"])
    np.testing.assert_array_equal(x[:, [6 * N, 7 * N - 1]], r["u0"])


def against_host(r, h, N, floor=0.0):
    """the GPU's records r against the host emulation's h; returns the largest multiplier
    difference, relative to the row's largest multiplier (or to floor where that is larger:
    gradient_floor)"""
    np.testing.assert_array_equal(r["status"], h["status"])
    np.testing.assert_array_equal(r["iters"], h["iters"])
    nx = 8 * N - 2
    assert np.abs(r["sol"][:, :nx] - h["sol"][:, :nx]).max() <= X_ATOL
    mg, mh = r["sol"][:, nx:], h["sol"][:, nx:]  # (z_L | z_U | lambda)
    assert (mg[:, :2 * nx] >= 0).all()
    return (np.abs(mg - mh).max(axis=1) / np.maximum(np.abs(mh).max(axis=1), floor)).max()


def gradient_floor(name, P):
    """The general sets hold the all-zero problem started at v = REF_V.  Its solution is its start:
    grad f = 0, no bound is active, so lambda = 0 and z is the barrier's mu / slack, 5e-9.  What the
    solver returns for lambda there is the rounding of the gradient's two cancelling terms,
    2 W_V v - 2 W_V REF_V = 200 - 200 (measured: |lambda| <= 1.9e-13 on the host, where the numpy
    certificate's stationarity residual of the same record is 1.1e-14; two host builds that
    contract other multiply-adds differ by 7.8e-15 in lambda, 1.5e-6 of the row's 5e-9, and so
    does an MI355X from the host: 1.546e-6 at N = 20, 1.466e-6 on the bicycle, printed by the
    test), so the scale a difference is measured against is not below those terms' size on these
    sets.  With it the sets' figures are 5.9e-16 and 4.0e-16.  Every other row's largest
    multiplier is above the floor (asserted).  0 for the other shapes: their measure is unchanged."""
    return 2.0 * P["W_V"] * P["REF_V"] if name.startswith("general_") else 0.0


def shape_cases(infinity_golden):
    """name: (P, state, coeffs) -- the fixture batches of the shapes below."""
    inf = infinity_golden
    cases = {"N20": (params_from_array(inf["params"]), inf["state"], inf["coeffs"])}
    P40, g40 = fixture_set("variants_N40")
    cases["N40"] = (P40, g40["state"], g40["coeffs"])
    P65, g65 = fixture_set("resto_N65")  # (its one row restores; the infinity rows at its horizon beside it)
    cases["N65"] = (P65, np.r_[g65["state"], inf["state"][:15]], np.r_[g65["coeffs"], inf["coeffs"][:15]])
    Pb, gb = fixture_set("bicycle_N25")
    cases["bicycle_N25"] = (Pb, gb["state"][:32], gb["coeffs"][:32])
    Pr, gr = fixture_set("resto_N20")
    cases["resto_N20"] = (Pr, gr["state"], gr["coeffs"])
    for name in ("general_N20", "general_bicycle_N25"):  # (problems away from the infinity course)
        Pg, gg = fixture_set(name)
        cases[name] = (Pg, gg["state"], gg["coeffs"])
    return cases


@pytest.fixture(scope="module")
def host_records(oracle, infinity_golden, tmp_path_factory):
    """The host emulation's records of every shape, computed once and left unchanged."""
    exe = build("wide_sol_check")
    out = {}
    for name, (P, st, cf) in shape_cases(infinity_golden).items():
        st, cf = np.ascontiguousarray(st), np.ascontiguousarray(cf)
        h = run_sol_harness(exe, P, st, cf, oracle.ref_opts(int(P["STEPS"])))
        h.update(P=P, state=st, coeffs=cf)
        out[name] = h
    return out


@pytest.mark.parametrize("name,park_capacity", [("N20", 0), ("N40", 0), ("N65", 0), ("bicycle_N25", 0), ("resto_N20", 0),
                                                ("resto_N20", 1), ("general_N20", 0), ("general_bicycle_N25", 0)])
def test_record_equals_the_host_emulations(torch_cuda, host_records, name, park_capacity):  # noqa: F811
    """N = 20 (split), 40 (unsplit), 65 (two stage blocks), the bicycle at N = 25, and rows that
    enter the restoration phase: written by the parked-problem kernel, and (a park area of one
    entry) by the overflow re-solve."""
    h = host_records[name]
    N = int(h["P"]["STEPS"])
    s = solver_for(h["P"])
    s.set_park_capacity(park_capacity)
    r = gpu_solve(torch_cuda, s, h["state"], h["coeffs"])
    if name == "resto_N20":
        assert (r["diag"][:, 0] > 0).all()
        d2 = r["diag"][:, 2]  # (1: continued by the parked-problem kernel, 2: solved again after an overflow)
        assert (d2 == 1).all() if park_capacity == 0 else ((d2 == 2).sum() >= len(d2) - 1 and (d2 >= 1).all())
    self_consistent(r, N)
    floor = gradient_floor(name, h["P"])
    big = np.abs(h["sol"][:, 8 * N - 2:]).max(axis=1)
    assert ((big >= floor) | (big < 1e-6)).all()  # (the floor acts on the rows without a multiplier alone)
    d = against_host(r, h, N, floor)
    print(f"{name} park {park_capacity}: multipliers rel {d:.3e} over {len(r['status'])} rows")
    if floor:
        print(f"   (relative to the row's largest multiplier alone: {against_host(r, h, N):.3e})")
    assert d <= MULT_REL_BOUND


def test_rows_and_an_invalid_row(torch_cuda, host_records, oracle, tmp_path_factory):  # noqa: F811
    """params_rows: two different rows and an invalid one.  Each valid problem's record is the host
    emulation's under its own row's parameters; the invalid row ends with status 13 and zeros."""
    from mpc_ros_amd import params

    h = host_records["N20"]
    P = h["P"]
    P2 = dict(P, REF_V=0.7 * P["REF_V"], W_CTE=2.0 * P["W_CTE"], ANGVEL=0.5 * P["ANGVEL"])
    st, cf = h["state"][:3], h["coeffs"][:3]
    rows = params.rows([P, P2, P])
    rows[2] = 0.0
    r = gpu_solve(torch_cuda, solver_for(dict(P, REF_V=0.1, W_V=7.0)), st, cf, rows=rows)
    assert r["status"][2] == 13 and (r["sol"][2] == 0).all() and (r["u0"][2] == 0).all()
    exe = build("wide_sol_check")
    for b, Pb in ((0, P), (1, P2)):
        hb = run_sol_harness(exe, Pb, st[b:b + 1], cf[b:b + 1], oracle.ref_opts(20))
        rb = {k: v[b:b + 1] for k, v in r.items()}
        self_consistent(rb, 20)
        assert against_host(rb, hb, 20) <= MULT_REL_BOUND


def test_fp32_configuration_reports_the_fp64_phase(torch_cuda):  # noqa: F811
    """dtype "fp32" at N = 40: the record comes from the fp64 phase (k_warm_wide and its resume
    workers), checked by the certificate at the fp64 phase's tolerances -- the reference's Ipopt
    defaults: dual_inf_tol 1, constr_viol_tol and compl_inf_tol 1e-4."""
    torch = torch_cuda
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=40)
    st, cf = infinity.make_problems(np.arange(64))
    s = solver_for(P, dtype="fp32")
    r = gpu_solve(torch, s, st, cf)
    assert set(r["diag"][:, 2]) <= {3, 4} and (r["diag"][:, 2] == 4).any()
    self_consistent(r, 40)
    cert = torch.empty((64, 4), dtype=torch.float64, device="cuda:0")
    s.kkt_device(dev(torch, st), dev(torch, cf), dev(torch, r["sol"]), cert)
    torch.cuda.synchronize()
    c = cert.cpu().numpy()
    ok = r["status"] == 1
    assert ok.sum() >= 48
    print(f"fp32 N = 40: dual {c[ok, 0].max():.3e} primal {c[ok, 1].max():.3e} compl {c[ok, 2].max():.3e}")
    assert c[ok, 0].max() <= 1.0 and c[ok, 1].max() <= 1e-4 and c[ok, 2].max() <= 1e-4
    np.testing.assert_allclose(c[:, 3], r["obj"], rtol=1e-10, atol=0)


def test_record_row_is_the_problems_own_in_an_ordered_batch(torch_cuda, infinity_golden):  # noqa: F811
    """2,049 problems (the infinity rows tiled): beyond 2,048 the batch is solved in
    expected-longest-first order, so the solve order is not the identity.  The record at row p is
    problem p's: tiled copies are bitwise equal, and x is the row's own u0 and traj."""
    g = infinity_golden
    P = params_from_array(g["params"])
    n = len(g["state"])
    idx = np.arange(2049) % n
    s = solver_for(P)
    r = gpu_solve(torch_cuda, s, g["state"][idx], g["coeffs"][idx])
    assert s.last_solve_order
    self_consistent(r, 20)
    for k in OUT + ("sol",):
        np.testing.assert_array_equal(r[k], r[k][:n][idx], err_msg=k)
    np.testing.assert_array_equal(r["status"][:n], g["status"])


def test_outputs_do_not_depend_on_the_record(torch_cuda, infinity_golden, features_golden):  # noqa: F811
    """sol=None leaves u0, traj, status, iters and obj bitwise what a solve with the record gives."""
    for g, n in ((infinity_golden, 64), (features_golden["resto_N20"], 4)):
        P = g["P"] if "P" in g else params_from_array(g["params"])
        s = solver_for(P)
        a = gpu_solve(torch_cuda, s, g["state"][:n], g["coeffs"][:n], want_sol=False)
        b = gpu_solve(torch_cuda, s, g["state"][:n], g["coeffs"][:n])
        for k in OUT + ("diag",):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_refusals_leave_the_handle_usable(torch_cuda, infinity_golden):  # noqa: F811
    """A null sol, and precision 1 with no_restoration 1: each returns -1 with mpcg_last_error set,
    before anything is launched, and the handle solves afterwards."""
    torch = torch_cuda
    from mpc_ros_amd import _lib
    from mpc_ros_amd.solver import solution_elems

    g = infinity_golden
    P = params_from_array(g["params"])
    st, cf = dev(torch, g["state"][:16]), dev(torch, g["coeffs"][:16])
    u0 = torch.zeros((16, 2), dtype=torch.float64, device="cuda:0")
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = solver_for(P)
    rc = L.mpcg_solve_device_sol(s._h, 16, p(st), p(cf), None, p(u0), None, None, None, None, None, None, None)
    assert rc == -1 and b"sol" in L.mpcg_last_error()
    with pytest.raises(_lib.MpcgError, match="sol is required"):
        _lib.check(L.mpcg_solve_sol(s._h, 16, None, None, None, None, None, None, None, None, None, None), "x")
    ref = gpu_solve(torch, s, g["state"][:16], g["coeffs"][:16])
    np.testing.assert_array_equal(ref["status"], g["status"][:16])
    s32 = solver_for(P, dtype="fp32", no_restoration=1)
    sol = torch.zeros((16, solution_elems(20)), dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.MpcgError, match="no fp64 ending"):
        s32.solve_device(st, cf, u0, sol=sol)
    assert (sol == 0).all()
    s32.solve_device(st, cf, u0)  # (the fp32 phase alone, without the record: as before)
    torch.cuda.synchronize()
    assert np.isfinite(u0.cpu().numpy()).all()


def test_host_buffer_call_returns_the_same_record(torch_cuda, infinity_golden):  # noqa: F811
    """BatchSolver.solve(want_solution=True) (mpcg_solve_sol, host buffers): the device call's bytes,
    with the handle's parameters and with a row per problem; x, zl, zu, lam are views of sol."""
    from mpc_ros_amd import params
    from mpc_ros_amd.solver import split_solution

    g = infinity_golden
    P = params_from_array(g["params"])
    st, cf = g["state"][:16], g["coeffs"][:16]
    s = solver_for(P)
    d = gpu_solve(torch_cuda, s, st, cf)
    for rows in (None, params.rows(P, B=16)):
        h = s.solve(st, cf, params_rows=rows, want_solution=True)
        for k in OUT + ("sol",):
            np.testing.assert_array_equal(h[k], d[k], err_msg=k)
        v = split_solution(h["sol"], 20)
        for k in ("x", "zl", "zu", "lam"):
            assert np.shares_memory(h[k], h["sol"]) and np.array_equal(h[k], v[k])
        assert h["x"].shape == (16, 158) and h["lam"].shape == (16, 120)


def test_cpp_class_keeps_the_solution_on_request(torch_cuda, tmp_path, infinity_golden):  # noqa: F811
    """MPC::keep_solution / solution() (tests/native/mpc_solution_check.cpp): nothing kept by
    default; with it on, the record of the same problem through the C-ABI, bit for bit."""
    import os
    import subprocess

    from conftest import ROOT

    exe = str(tmp_path / "mpc_solution")
    lib = os.path.join(ROOT, "mpc_ros_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "mpc_solution_check.cpp"), "-L", lib, "-lmpcg",
                           "-L/opt/rocm/lib", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    g = infinity_golden
    rows = [0, 7, 260]
    text = "\n".join(" ".join(repr(float(v)) for v in np.r_[g["state"][b], g["coeffs"][b]]) for b in rows) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
    assert out[0] == "kept 0"
    r = gpu_solve(torch_cuda, solver_for(params_from_array(g["params"])), g["state"][rows], g["coeffs"][rows])
    for i in range(len(rows)):
        vals = np.array(out[1 + i].split(), dtype=float)
        np.testing.assert_array_equal(vals[:2], r["u0"][i])
        np.testing.assert_array_equal(vals[2:], r["sol"][i])
