"""The feedback gains on the host (no GPU needed): mpcg_sens, the kernel's code with the 64 lanes in
a loop (mpc_ros_amd/csrc/mpcg_sens.h), on the records of the host emulation of the solver.

Two references, neither of which shares code with the sweep:
  * the dense solve of the definition's system (include/mpcg.h "Sensitivities of the solution") in
    numpy, built from the oracle's Hessian and dense Jacobian; the coefficient right-hand sides are
    central differences in c of the oracle's gradient, Jacobian and constraint values, which are
    linear in c.  The matrix is equilibrated by d = sqrt(max(|diag|, 1));
  * central differences of oracle solves (h = 1e-4, tol 1e-10, no iteration budget).

SENS_DENSE_MEASURED is the largest max |delta| / max(1, max |G|) of gain and dx against the dense
solve over DENSE_SETS' rows (test_against_the_dense_solve prints the figure of every set); the
bound is ten times it -- another elimination order rounds differently -- and never above 1e-6, the
level at which the dense solve itself agrees with finite differences.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_solution_host import nlp_bounds, records, split

# 3.286e-8 is bicycle_N25 row 61, whose equilibrated matrix has condition number 1.3e12 (a
# multiplier over a slack of 5e14 on its diagonal): against that row's dense solve refined with
# long-double residuals the dense solve itself is off by 3.29e-8 and the sweep by 5.7e-14.  Every
# other row of the six sets is within 8.4e-12.
SENS_DENSE_MEASURED = 3.286e-8
SENS_DENSE_BOUND = min(10 * SENS_DENSE_MEASURED, 1e-6)
FD_ATOL = 1e-4  # 20 x the 5.4e-6 between the dense solve and finite differences
FD_H = 1e-4
CVT, BRF = 1e-4, 1e-8  # constr_viol_tol, bound_relax_factor of the records' solves (Ipopt's defaults)

DENSE_SETS = {"variants_N3": None, "infinity": range(24), "variants_N40": None, "bicycle_N25": None,
              "resto_N65": None, "variants_N80": None, "general_N20": None, "general_bicycle_N25": None}


def dense_rows(name, r):
    """The status-1 rows of a set of DENSE_SETS."""
    sel = DENSE_SETS[name]
    return [b for b in (range(len(r["state"])) if sel is None else sel) if r["status"][b] == 1]


def kkt_matrix(oracle, P, coeffs, sol):
    """The definition's matrix of one record, and (W + Sigma, J) it is made of."""
    N = int(P["STEPS"])
    x, zl, zu, lam = split(sol, N)
    _, J, H = oracle.mpc_derivs(P, coeffs, x, 1.0, lam)
    if not np.array_equal(H, H.T):  # (a triangle only)
        assert not np.triu(H, 1).any() or not np.tril(H, -1).any()
        H = H + H.T - np.diag(np.diag(H))
    xl, xu, _ = nlp_bounds(P, np.zeros(6))
    rl = np.minimum(CVT, BRF * np.maximum(1.0, np.abs(xu)))
    sig = zl / (x - (xl - rl)) + zu / ((xu + rl) - x)
    nx, ng = 8 * N - 2, 6 * N
    K = np.zeros((nx + ng, nx + ng))
    K[:nx, :nx] = H + np.diag(sig)
    K[:nx, nx:] = J.T
    K[nx:, :nx] = J
    return K


def rhs(oracle, P, coeffs, sol):
    """The ten right-hand sides [nx + ng, 10]."""
    N = int(P["STEPS"])
    nx, ng = 8 * N - 2, 6 * N
    x, _, _, lam = split(sol, N)
    R = np.zeros((nx + ng, 10))
    for s in range(6):
        R[nx + s * N, s] = 1.0
    for i in range(4):
        def at(c):
            gf, J, _ = oracle.mpc_derivs(P, c, x, 1.0, lam)
            return np.r_[gf + J.T @ lam, oracle.mpc_fg(P, c, x)[1:]]
        e = np.zeros(4)
        e[i] = 1.0
        R[:, 6 + i] = -(at(coeffs + e) - at(coeffs - e)) / 2.0
    return R


def inertia(Ks):
    ev = np.linalg.eigvalsh(Ks)
    return int((ev > 0).sum()), int((ev < 0).sum())


def dense_reference(oracle, P, coeffs, sol):
    """(gain [2, 10], dx [10, nx], inertia) of one record by the equilibrated dense solve."""
    N = int(P["STEPS"])
    nx = 8 * N - 2
    K = kkt_matrix(oracle, P, coeffs, sol)
    d = np.sqrt(np.maximum(np.abs(np.diag(K)), 1.0))
    Ks = K / d[:, None] / d[None, :]
    y = np.linalg.solve(Ks, rhs(oracle, P, coeffs, sol) / d[:, None]) / d[:, None]
    dx = np.ascontiguousarray(y[:nx].T)
    return dx[:, [6 * N, 7 * N - 1]].T.copy(), dx, inertia(Ks)


def host_sens(libmpcg, r, rows_idx=None, sol=None, **kw):
    from mpc_ros_amd import solver

    idx = np.arange(len(r["state"])) if rows_idx is None else np.asarray(rows_idx)
    return solver.sens(dict(r["P"]), r["state"][idx], r["coeffs"][idx], r["sol"][idx] if sol is None else sol, **kw)


_dense = {}


def dense_set(name, oracle, tmp_path_factory):
    """Computed once per set and shared (tests/test_gpu_sens.py too), never modified: the rows, and
    the dense reference's gain, dx and inertia of each."""
    if name not in _dense:
        r = records(name, oracle, tmp_path_factory)
        rows = dense_rows(name, r)
        ref = [dense_reference(oracle, r["P"], r["coeffs"][b], r["sol"][b]) for b in rows]
        out = dict(rows=np.array(rows), gain=np.array([g for g, _, _ in ref]), dx=np.array([d for _, d, _ in ref]),
                   inertia=[i for _, _, i in ref])
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _dense[name] = out
    return _dense[name]


def rel_err(gain, dx, ref_gain, ref_dx):
    """max |delta| / max(1, max |G|) per row, over gain and dx."""
    scale = np.maximum(1.0, np.abs(ref_gain).max(axis=(1, 2)))
    return np.maximum(np.abs(gain - ref_gain).max(axis=(1, 2)), np.abs(dx - ref_dx).max(axis=(1, 2))) / scale


@pytest.mark.parametrize("name", list(DENSE_SETS))
def test_against_the_dense_solve(libmpcg, oracle, tmp_path_factory, name):
    r = records(name, oracle, tmp_path_factory)
    N = r["N"]
    ref = dense_set(name, oracle, tmp_path_factory)
    assert len(ref["rows"]) >= 1
    for b, i in zip(ref["rows"], ref["inertia"]):
        assert i == (8 * N - 2, 6 * N), (name, b, i)
    got = host_sens(libmpcg, r, ref["rows"], want_dx=True)
    e = rel_err(got["gain"], got["dx"], ref["gain"], ref["dx"])
    print(f"{name}: {len(ref['rows'])} rows, max |G| {np.abs(ref['gain']).max():.3e}, "
          f"max |delta| / max(1, max|G|) = {e.max():.3e} (bound {SENS_DENSE_BOUND:.1e})")
    assert (got["info"] == 0).all()
    assert (e <= SENS_DENSE_BOUND).all()
    # dx's rows 6N and 7N - 1 are the gain, and the state columns start from the unit vectors
    np.testing.assert_array_equal(got["dx"][:, :, [6 * N, 7 * N - 1]].transpose(0, 2, 1), got["gain"])
    np.testing.assert_array_equal(got["dx"][:, :6, 0:6 * N:N], np.broadcast_to(np.eye(6), (len(e), 6, 6)))


def test_against_finite_differences_of_the_oracle(libmpcg, oracle, tmp_path_factory):
    r = records("infinity", oracle, tmp_path_factory)
    rows = list(range(24))
    assert (r["status"][rows] == 1).all()
    got = host_sens(libmpcg, r, rows)
    assert (got["info"] == 0).all()
    o = oracle.ipm_opts(tol=1e-10, cpu_iter_budget=-1)
    worst = 0.0
    for n, b in enumerate(rows):
        fd = np.zeros((2, 10))
        for c in range(10):
            u = []
            for sgn in (1.0, -1.0):
                st, cf = r["state"][b].copy(), r["coeffs"][b].copy()
                (st if c < 6 else cf)[c if c < 6 else c - 6] += sgn * FD_H
                q = oracle.mpc_solve(r["P"], st, cf, opts=o)
                assert q["status"] == 1, (b, c, sgn)
                u.append(q["u0"])
            fd[:, c] = (u[0] - u[1]) / (2 * FD_H)
        d = np.abs(got["gain"][n] - fd).max()
        worst = max(worst, d)
        assert d <= FD_ATOL, (b, d)
    print(f"infinity rows 0..23: max |gain - FD| = {worst:.3e} (bound {FD_ATOL:.0e})")


def test_a_transposed_or_missigned_gain_fails(libmpcg, oracle, tmp_path_factory):
    """The negative control of test_against_the_dense_solve on infinity row 1."""
    r = records("infinity", oracle, tmp_path_factory)
    ref = dense_set("infinity", oracle, tmp_path_factory)
    i = int(np.flatnonzero(ref["rows"] == 1)[0])
    g = host_sens(libmpcg, r, [1])["gain"][0]
    scale = max(1.0, np.abs(ref["gain"][i]).max())
    assert np.abs(g - ref["gain"][i]).max() / scale <= SENS_DENSE_BOUND
    swapped = g[::-1]
    negated = g.copy()
    negated[:, 6:] *= -1.0
    assert np.abs(swapped - ref["gain"][i]).max() / scale > SENS_DENSE_BOUND
    assert np.abs(negated - ref["gain"][i]).max() / scale > SENS_DENSE_BOUND


def flag_records(r):
    """The four flag records of infinity row 1 and what each must give: (sols [4, ne], parameter
    rows [4, 16], expected info [4])."""
    from mpc_ros_amd import params

    N, nx = r["N"], 8 * r["N"] - 2
    sols = np.repeat(r["sol"][1][None], 4, axis=0)
    # 0: every lambda of the x rows 1e6, zl = zu = 0: the wrong inertia
    sols[0, nx:3 * nx] = 0.0
    sols[0, 3 * nx:3 * nx + N] = 1e6
    # 1: one NaN
    sols[1, 3 * N + 2] = np.nan
    # 2: a parameter row with DT = 0
    rows = params.rows(r["P"], 4)
    rows[2, 0] = 0.0
    # 3: x outside its relaxed bound (the first angular velocity past ANGVEL + the relaxation)
    sols[3, 6 * N] = r["P"]["ANGVEL"] + 1e-3
    return sols, rows, np.array([1, 2, 2, 2], dtype=np.int32)


def test_flags(libmpcg, oracle, tmp_path_factory):
    r = records("infinity", oracle, tmp_path_factory)
    N = r["N"]
    sols, rows, want = flag_records(r)
    K = kkt_matrix(oracle, r["P"], r["coeffs"][1], sols[0])
    d = np.sqrt(np.maximum(np.abs(np.diag(K)), 1.0))
    assert inertia(K / d[:, None] / d[None, :]) != (8 * N - 2, 6 * N)
    # in one batch with good rows around them: the neighbours are unaffected
    idx = [0, 1, 1, 1, 1, 2]
    batch = np.concatenate([r["sol"][[0]], sols, r["sol"][[2]]])
    all_rows = np.concatenate([rows[[0]], rows, rows[[0]]])
    got = host_sens(libmpcg, r, idx, sol=batch, params_rows=all_rows, want_dx=True)
    np.testing.assert_array_equal(got["info"], np.r_[0, want, 0])
    assert np.isnan(got["gain"][1:5]).all() and np.isnan(got["dx"][1:5]).all()
    good = host_sens(libmpcg, r, [0, 2], want_dx=True)
    np.testing.assert_array_equal(got["gain"][[0, 5]], good["gain"])
    np.testing.assert_array_equal(got["dx"][[0, 5]], good["dx"])


def test_rows_equal_the_handles_parameters(libmpcg, oracle, tmp_path_factory):
    import ctypes as C

    from mpc_ros_amd import _lib, solver

    for name in ("infinity", "bicycle_N25"):
        r = records(name, oracle, tmp_path_factory)
        B = 6
        p = solver._params_struct(dict(r["P"]), "fp64", {})
        rows = np.zeros((B, _lib.PP_FIELDS))
        assert libmpcg.mpcg_pparams_fill(C.byref(p), B, rows.ctypes.data_as(C.POINTER(C.c_double))) == 0
        a = host_sens(libmpcg, r, range(B), want_dx=True)
        b = host_sens(libmpcg, r, range(B), params_rows=rows, want_dx=True)
        for k in ("gain", "dx", "info"):
            np.testing.assert_array_equal(a[k], b[k])


def test_refusals(libmpcg, oracle, tmp_path_factory):
    import ctypes as C

    from mpc_ros_amd import solver

    r = records("variants_N3", oracle, tmp_path_factory)
    p = solver._params_struct(dict(r["P"]), "fp64", {})
    dp = C.POINTER(C.c_double)
    st, cf, so = (np.ascontiguousarray(r[k][:1]) for k in ("state", "coeffs", "sol"))
    g = np.zeros((1, 2, 10))
    a = [st.ctypes.data_as(dp), cf.ctypes.data_as(dp), None]
    assert libmpcg.mpcg_sens(C.byref(p), 1, *a, None, g.ctypes.data_as(dp), None, None) == -1
    assert libmpcg.mpcg_sens(C.byref(p), 1, *a, so.ctypes.data_as(dp), None, None, None) == -1
    assert libmpcg.mpcg_sens(C.byref(p), 1, *a, so.ctypes.data_as(dp), g.ctypes.data_as(dp), None, None) == 0


def run_sens_check(exe, r, rows_idx):
    from mpc_ros_amd import params

    P = r["P"]
    row = params.rows(P, 1)[0]
    lines = [f"{int(P.get('MODEL', 0))} {r['N']} {len(rows_idx)} {CVT!r} {BRF!r}", " ".join(repr(float(v)) for v in row)]
    for b in rows_idx:
        lines.append(" ".join(repr(float(v)) for v in np.r_[r["coeffs"][b], r["sol"][b]]))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.strip().split("\n")
    vals = np.array([ln.split() for ln in out[:-1]], dtype=np.float64)
    nx = 8 * r["N"] - 2
    return dict(info=vals[:, 0].astype(np.int32), gain=vals[:, 1:21].reshape(-1, 2, 10),
                dx=vals[:, 21:].reshape(-1, 10, nx)), np.array(out[-1].split(), dtype=np.float64)


def test_sweeps_under_sanitizers(libmpcg, oracle, tmp_path_factory, tmp_path):
    """tests/native/sens_check.cpp: a stand-alone program over mpcg_sens.h, built with ASan and
    UBSan and run directly on the N = 3 and N = 65 records; what it prints is mpcg_sens's result."""
    exe = str(tmp_path / "sens_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'mpc_ros_amd', 'csrc')}", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sens_check.cpp")])
    for name in ("variants_N3", "resto_N65"):
        r = records(name, oracle, tmp_path_factory)
        idx = list(range(min(4, len(r["state"]))))
        got, _ = run_sens_check(exe, r, idx)
        want = host_sens(libmpcg, r, idx, want_dx=True)
        np.testing.assert_array_equal(got["info"], want["info"])
        for k in ("gain", "dx"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-300, equal_nan=True)


def apply_rule(P, gain, u0, dstate, dcoeffs=None, rows=None):
    """mpcg_sens_apply's rule in numpy, in its order of additions."""
    B = len(u0)
    u = np.zeros((B, 2))
    for b in range(B):
        lim = (rows[b, 11], rows[b, 12]) if rows is not None else (P["ANGVEL"], P["MAXTHR"])
        for i in range(2):
            a = 0.0
            for j in range(6):
                a += gain[b, i, j] * dstate[b, j]
            if dcoeffs is not None:
                for j in range(4):
                    a += gain[b, i, 6 + j] * dcoeffs[b, j]
            v = u0[b, i] + a
            u[b, i] = u0[b, i] if not np.isfinite(v) else min(max(v, -lim[i]), lim[i])
    return u


def apply_case(r, gain):
    """Inputs of the correction rule that reach every branch: small and large deviations (the
    large ones clip at either bound), a NaN gain, rows with their own limits."""
    from mpc_ros_amd import params

    B = len(gain)
    rng = np.random.default_rng(7)
    g = np.array(gain)
    g[2] = np.nan
    u0 = rng.uniform(-0.5, 0.5, (B, 2))
    ds = rng.normal(0, 0.02, (B, 6))
    ds[3:6] *= 50.0
    dc = rng.normal(0, 0.02, (B, 4))
    rows = params.rows(r["P"], B)
    rows[1::2, 11] = 0.3
    rows[1::2, 12] = 0.2
    return g, u0, ds, dc, rows


def test_the_correction_rule(libmpcg, oracle, tmp_path_factory):
    from mpc_ros_amd import solver

    r = records("infinity", oracle, tmp_path_factory)
    P = dict(r["P"])
    g, u0, ds, dc, rows = apply_case(r, host_sens(libmpcg, r, range(12))["gain"])
    for kw in (dict(dcoeffs=dc), dict(), dict(dcoeffs=dc, rows=rows)):
        u = solver.sens_apply(P, g, u0, ds, dcoeffs=kw.get("dcoeffs"), params_rows=kw.get("rows"))
        want = apply_rule(P, g, u0, ds, **kw)
        np.testing.assert_array_equal(u, want)
        lim = rows[:, 11:13] if "rows" in kw else np.broadcast_to([P["ANGVEL"], P["MAXTHR"]], u.shape)
        ok = np.arange(len(u)) != 2
        assert (np.abs(u[ok]) <= lim[ok]).all()
        np.testing.assert_array_equal(u[2], u0[2])  # a NaN gain: u0
    u = solver.sens_apply(P, g, u0, ds, dcoeffs=dc)
    assert (np.abs(u) == np.array([P["ANGVEL"], P["MAXTHR"]])).any()  # (the case does clip)
    assert not np.array_equal(u, solver.sens_apply(P, g, u0, ds))
