"""Start point in, on the host (no GPU needed).

tests/native/wide_start_check.cpp runs mpc_ros_amd/csrc/wide_core.h on 64 fibers, every problem
started by WideSolver::init_start from a solution record in its own mode (include/mpcg.h
MPCG_START_*); it does not compile without init_start.  tests/native/start_oracle.c is the oracle
solved from a caller's starting point (built here against liboracle.so).

The shapes are SHAPES below.  The neighbour problem of row b is row b with state[3:6] +=
(0.02, 0.01, -0.01) and coeffs[0] += 0.01; its start record is the cold solution of row b.

Iterations over the neighbour problems of each shape, FULL at mu0 = 1e-4 / PRIMAL / cold (the tests
print them; DESIGN.md "Start point in"): infinity_N20 313 / 540 / 864, variants_N40 153 / 267 / 500,
resto_N65 87 / 152 / 307, bicycle_N25 181 / 332 / 623, variants_N3 64 / 99 / 112, resto_N20 69 / 69 /
182.  |u0 - u0_cold| of the FULL starts: U0_DIFF_MEASURED.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_harness import build, harness_stdin, opts_line
from test_solution_host import fixture_set, split

SHIM = os.path.join(ROOT, "tests", "native", "start_oracle.c")
COLD, PRIMAL, FULL = 0, 1, 2
X_ATOL = 1e-7   # the cold parity tests' bound on x
MU0 = 1e-4      # class MPC's default barrier parameter of a FULL start
# rows the oracle comparison may leave out: those on which the oracle's own iteration count differs
# between kkt_structured 0 and 1 for that start
SKIP_CAP = {"infinity_N20": 2}
# the largest |u0(FULL start) - u0(cold solve)| over the neighbour problems of all shapes, measured
# on the host emulation (printed by test_full_on_neighbours), and the bound: ten times it
U0_DIFF_MEASURED = 2.1e-8
U0_DIFF_BOUND = 10 * U0_DIFF_MEASURED

SHAPES = ["infinity_N20", "variants_N40", "resto_N65", "bicycle_N25", "variants_N3", "resto_N20"]


def shape(name):
    """(parameter dict, state, coeffs) of a shape."""
    if name == "infinity_N20":
        P, g = fixture_set("infinity")
        return P, np.ascontiguousarray(g["state"][:64]), np.ascontiguousarray(g["coeffs"][:64])
    if name == "bicycle_N25":
        P, g = fixture_set("bicycle_N25")
        return P, np.ascontiguousarray(g["state"][:32]), np.ascontiguousarray(g["coeffs"][:32])
    if name == "resto_N65":  # (two stage blocks: the restoration row and 15 infinity rows at N = 65)
        P, g = fixture_set("resto_N65")
        _, gi = fixture_set("infinity")
        return (P, np.ascontiguousarray(np.r_[g["state"], gi["state"][:15]]),
                np.ascontiguousarray(np.r_[g["coeffs"], gi["coeffs"][:15]]))
    P, g = fixture_set(name)
    return P, np.ascontiguousarray(g["state"]), np.ascontiguousarray(g["coeffs"])


def neighbour(state, coeffs):
    s, c = state.copy(), coeffs.copy()
    s[:, 3:6] += (0.02, 0.01, -0.01)
    c[:, 0] += 0.01
    return s, c


def cold_point(state, N):
    """MPC::Solve's own start as a record: zeros, the state in stage 0."""
    rec = np.zeros((len(state), 3 * (8 * N - 2) + 6 * N))
    for s in range(6):
        rec[:, s * N] = state[:, s]
    return rec


def run_start(exe, P, state, coeffs, o, modes, starts, mu0=MU0, cold_scaling=0):
    N, B = int(P["STEPS"]), len(state)
    modes = np.broadcast_to(np.asarray(modes, dtype=np.int64), (B,))
    mu0 = np.broadcast_to(np.asarray(mu0, dtype=np.float64), (B,))
    tail = [str(int(cold_scaling))]
    for b in range(B):
        tail.append(f"{int(modes[b])} {float(mu0[b])!r}")
        tail.append(" ".join(repr(float(v)) for v in starts[b]))
    text = harness_stdin(P, state, coeffs, o, opts_line(o)) + "\n".join(tail) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    rows = np.array([r.split() for r in out.strip().split("\n")], dtype=np.float64)
    ne = 3 * (8 * N - 2) + 6 * N
    assert rows.shape == (B, 10 + 3 * N + ne)
    return dict(status=rows[:, 0].astype(int), iters=rows[:, 1].astype(int), used=rows[:, 2].astype(int),
                diag=rows[:, 3:6].astype(int), sf=rows[:, 6], obj=rows[:, 7], u0=rows[:, 8:10],
                traj=rows[:, 10:10 + 3 * N], sol=np.ascontiguousarray(rows[:, 10 + 3 * N:]))


def same_bits(a, b, keys=("status", "iters", "diag", "obj", "u0", "traj", "sol"), rows=slice(None)):
    for k in keys:
        np.testing.assert_array_equal(a[k][rows], b[k][rows], err_msg=k)


_cache = {}


def case(name, oracle, tmp_path_factory):
    """Computed once per shape and shared, never modified: the cold solves of the shape's rows (the
    start records) and of their neighbour problems, by the harness in COLD mode."""
    if name not in _cache:
        P, state, coeffs = shape(name)
        N = int(P["STEPS"])
        o = oracle.ref_opts(N)
        exe = build("wide_start_check")
        zero = np.zeros((len(state), 3 * (8 * N - 2) + 6 * N))
        cold = run_start(exe, P, state, coeffs, o, COLD, zero)
        ns, nc = neighbour(state, coeffs)
        ncold = run_start(exe, P, ns, nc, o, COLD, zero)
        r = dict(P=P, N=N, opts=o, exe=exe, state=state, coeffs=coeffs, cold=cold, nstate=ns, ncoeffs=nc,
                 ncold=ncold)
        for d in (cold, ncold):
            for v in d.values():
                v.setflags(write=False)
        _cache[name] = r
    return _cache[name]


@pytest.fixture(params=SHAPES)
def cs(request, oracle, tmp_path_factory):
    return request.param, case(request.param, oracle, tmp_path_factory)


# ---------------------------------------------------------------- the shim oracle
_shim = []


def shim(oracle, tmp_path_factory):
    if not _shim:
        so = str(tmp_path_factory.mktemp("shim") / "libstart_oracle.so")
        odir = os.path.dirname(oracle.LIB_PATH)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'oracle')}", "-o", so, SHIM,
                               f"-L{odir}", "-loracle", f"-Wl,-rpath,{odir}"])
        oracle.lib()  # (liboracle.so is loaded first: the shim resolves against it)
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        L.start_oracle_solve.argtypes = [C.POINTER(oracle.MpcParams), C.POINTER(oracle.IpmOpts), dp, dp, dp, dp,
                                         C.POINTER(C.c_int)]
        _shim.append(L)
    return _shim[0]


def oracle_from(oracle, L, P, o, state, coeffs, x0, structured):
    N = int(P["STEPS"])
    p = oracle.params_from_dict(P)
    oo = oracle.IpmOpts.from_buffer_copy(o)
    oo.kkt_structured = structured
    st, it, xs = [], [], []
    for b in range(len(state)):
        x = np.zeros(8 * N - 2)
        n = C.c_int()
        s = L.start_oracle_solve(C.byref(p), C.byref(oo), oracle._dp(np.ascontiguousarray(state[b])),
                                 oracle._dp(np.ascontiguousarray(coeffs[b])), oracle._dp(np.ascontiguousarray(x0[b])),
                                 oracle._dp(x), C.byref(n))
        st.append(s)
        it.append(n.value)
        xs.append(x)
    return np.array(st), np.array(it), np.array(xs)


# ---------------------------------------------------------------- 1. PRIMAL from the cold point
def test_primal_from_cold_point_is_the_cold_solve(cs):
    name, r = cs
    got = run_start(r["exe"], r["P"], r["state"], r["coeffs"], r["opts"], PRIMAL, cold_point(r["state"], r["N"]))
    print(f"{name}: start_used {np.unique(got['used'], return_counts=True)}; restoration phases "
          f"{r['cold']['diag'][:, 0].sum()}")
    # every row of every shape runs in PRIMAL mode: none is carried by the cold fall-back (-2, a
    # Jacobian entry above 100 at the cold point)
    assert (got["used"] == PRIMAL).all()
    same_bits(got, r["cold"])
    np.testing.assert_array_equal(got["sf"], r["cold"]["sf"])
    if name == "resto_N20":
        assert (r["cold"]["diag"][:, 0] > 0).any()


def test_cold_mode_is_the_solution_harness(oracle, tmp_path_factory):
    """The COLD rows against tests/native/wide_sol_check.cpp, which knows no start."""
    from test_solution_host import run_sol_harness

    for name in ("variants_N3", "resto_N20"):
        r = case(name, oracle, tmp_path_factory)
        ref = run_sol_harness(build("wide_sol_check"), r["P"], r["state"], r["coeffs"], r["opts"])
        for k in ("status", "iters", "obj", "u0", "sol"):
            np.testing.assert_array_equal(r["cold"][k], ref[k], err_msg=k)
        assert (r["cold"]["used"] == COLD).all()


# ------------------------------------------------ 1b. restoration from a start that is not the cold point
def restoring_starts(r):
    """Eight problems on the resto_N20 rows whose starts are not the cold point and of which two
    enter the restoration phase (RESTORING): rows 0..3 in FULL mode from the cold point with z =
    1 / sf, lambda = 0 and mu0 = MU0 (row 1 restores; its cold solve takes other iterates: 80
    iterations against 70), rows 4..7 the same problems in PRIMAL mode from the cold point with the
    turn rate of stage N - 2 at 1.01 max|grad f| / (2 (W_ANGVEL + W_DANGVEL)) -- beyond its bound,
    pushed back inside after the scaling was taken there: the objective scale is the cold one /
    1.01 (row 6 restores).  Returns (state, coeffs, modes, starts)."""
    N, P = r["N"], r["P"]
    nx = 8 * N - 2
    st, cf, sf = r["state"], r["coeffs"], r["cold"]["sf"]
    full = cold_point(st, N)
    full[:, nx:3 * nx] = (1.0 / sf)[:, None]
    prim = cold_point(st, N)
    prim[:, 6 * N + N - 2] = 1.01 * (100.0 / sf) / (2.0 * (P["W_ANGVEL"] + P["W_DANGVEL"]))
    modes = np.array([FULL] * 4 + [PRIMAL] * 4, dtype=np.int32)
    return (np.ascontiguousarray(np.r_[st, st]), np.ascontiguousarray(np.r_[cf, cf]), modes,
            np.ascontiguousarray(np.r_[full, prim]))


RESTORING = [1, 6]


def test_restoration_from_a_start_that_is_not_the_cold_point(oracle, tmp_path_factory):
    """The park / unpark path of the harness with a started solve's state: the FULL row's iterates
    are not the cold solve's, and the PRIMAL row carries an objective scale that is not the cold one
    through the restoration phase."""
    r = case("resto_N20", oracle, tmp_path_factory)
    st, cf, modes, starts = restoring_starts(r)
    h = run_start(r["exe"], r["P"], st, cf, r["opts"], modes, starts, mu0=MU0)
    cold = r["cold"]
    print(f"restoration phases {h['diag'][:, 0]}, iterations {h['iters']} (cold {cold['iters']}), "
          f"sf / cold sf {h['sf'] / np.r_[cold['sf'], cold['sf']]}")
    np.testing.assert_array_equal(h["used"], modes)
    np.testing.assert_array_equal(np.flatnonzero(h["diag"][:, 0] > 0), RESTORING)
    np.testing.assert_array_equal(h["status"], 1)
    assert h["iters"][1] != cold["iters"][1]
    np.testing.assert_allclose(h["sf"][4:], cold["sf"] / 1.01, rtol=1e-12)
    np.testing.assert_array_equal(h["sf"][:4], cold["sf"])
    # the same minimum as the cold solve on the restoring rows
    assert np.abs(h["u0"][RESTORING] - np.r_[cold["u0"], cold["u0"]][RESTORING]).max() <= 1e-6


# ---------------------------------------------------------------- 2. PRIMAL against the oracle
def test_primal_on_neighbours_equals_the_oracle(cs, oracle, tmp_path_factory):
    name, r = cs
    N, P, o = r["N"], r["P"], r["opts"]
    x0 = split(r["cold"]["sol"], N)[0]
    got = run_start(r["exe"], P, r["nstate"], r["ncoeffs"], o, PRIMAL, r["cold"]["sol"])
    L = shim(oracle, tmp_path_factory)
    st0, it0, xs0 = oracle_from(oracle, L, P, o, r["nstate"], r["ncoeffs"], x0, 0)
    _, it1, _ = oracle_from(oracle, L, P, o, r["nstate"], r["ncoeffs"], x0, 1)
    moves = it0 != it1  # the oracle's own count moves with its linear algebra
    keep = ~moves
    d = np.abs(split(got["sol"], N)[0] - xs0).max(axis=1)
    print(f"{name}: start_used {np.unique(got['used'], return_counts=True)}; left out {np.flatnonzero(moves)}; "
          f"max |x - oracle x| = {d[keep].max():.3e}; iterations {got['iters'].sum()} (cold {r['ncold']['iters'].sum()})")
    assert moves.sum() <= SKIP_CAP.get(name, 1)
    assert (got["used"] == PRIMAL).all()
    np.testing.assert_array_equal(got["status"][keep], st0[keep])
    np.testing.assert_array_equal(got["iters"][keep], it0[keep])
    assert d[keep].max() <= X_ATOL


def test_primal_with_the_cold_scaling_differs_from_the_oracle(oracle, tmp_path_factory):
    """The negative control: the same starts with the scaling of the cold setup()."""
    L = shim(oracle, tmp_path_factory)
    n_sf, n_diff = 0, 0
    for name in SHAPES:
        r = case(name, oracle, tmp_path_factory)
        N, P, o = r["N"], r["P"], r["opts"]
        good = run_start(r["exe"], P, r["nstate"], r["ncoeffs"], o, PRIMAL, r["cold"]["sol"])
        rows = np.flatnonzero(good["sf"] != r["ncold"]["sf"])
        if not len(rows):
            continue
        n_sf += len(rows)
        sub = lambda a: np.ascontiguousarray(a[rows])
        bad = run_start(r["exe"], P, sub(r["nstate"]), sub(r["ncoeffs"]), o, PRIMAL, sub(r["cold"]["sol"]),
                        cold_scaling=1)
        st0, it0, xs0 = oracle_from(oracle, L, P, o, sub(r["nstate"]), sub(r["ncoeffs"]),
                                    split(sub(r["cold"]["sol"]), N)[0], 0)
        d = np.abs(split(bad["sol"], N)[0] - xs0).max(axis=1)
        n_diff += int(((bad["status"] != st0) | (bad["iters"] != it0) | (d > X_ATOL)).sum())
    print(f"{n_sf} rows whose objective scale at the start differs from the cold one; {n_diff} of them differ "
          f"from the oracle under the cold scaling")
    assert n_sf >= 1 and n_diff >= 1


# ---------------------------------------------------------------- 3. FULL on the neighbours
_full_sums = {}
_full_du = {}


def test_full_on_neighbours(cs, libmpcg):
    from mpc_ros_amd import solver

    name, r = cs
    N, P, o = r["N"], r["P"], r["opts"]
    got = run_start(r["exe"], P, r["nstate"], r["ncoeffs"], o, FULL, r["cold"]["sol"], mu0=MU0)
    assert (got["used"] == FULL).all()
    ok = r["ncold"]["status"] == 1
    assert ok.any()
    np.testing.assert_array_equal(got["status"][ok], 1)
    cert = solver.kkt(dict(P), r["nstate"], r["ncoeffs"], got["sol"])
    du = np.abs(got["u0"] - r["ncold"]["u0"])[ok].max()
    s_full, s_cold = int(got["iters"].sum()), int(r["ncold"]["iters"].sum())
    _full_sums[name] = (s_full, s_cold)
    _full_du[name] = du
    print(f"{name}: iterations FULL {s_full} cold {s_cold}; max |u0 - u0_cold| = {du:.3e}; dual "
          f"{cert[ok, 0].max():.3e} primal {cert[ok, 1].max():.3e} compl {cert[ok, 2].max():.3e}")
    assert cert[ok, 0].max() <= o.dual_inf_tol
    assert cert[ok, 1].max() <= o.constr_viol_tol
    assert cert[ok, 2].max() <= o.compl_inf_tol
    assert du <= U0_DIFF_BOUND
    assert s_full < s_cold


# ---------------------------------------------------------------- 4. rejections
def test_bad_starts_are_solved_cold(oracle, tmp_path_factory):
    r = case("infinity_N20", oracle, tmp_path_factory)
    N, P, o = r["N"], r["P"], r["opts"]
    nx = 8 * N - 2
    rows = np.arange(8)
    sub = lambda a: np.ascontiguousarray(a[rows])
    state, coeffs = sub(r["nstate"]), sub(r["ncoeffs"])
    starts = sub(r["cold"]["sol"]).copy()
    modes = np.array([PRIMAL, FULL, FULL, PRIMAL, PRIMAL, FULL, FULL, PRIMAL])
    base = run_start(r["exe"], P, state, coeffs, o, modes, starts)
    np.testing.assert_array_equal(base["used"], modes)
    starts[0, 3 * N + 2] = np.nan          # a NaN in x, PRIMAL
    starts[1, nx + 5] = -1e-3              # a negative zl, FULL
    starts[2, 3 * nx + 7] = np.inf         # a non-finite lambda, FULL
    starts[3, 3 * nx + 7] = np.nan         # ... which PRIMAL does not read
    # |f'(x)| > 100 at the start's x of stage 1 (PRIMAL): c1 alone
    coeffs = coeffs.copy()
    coeffs[4, 1] = 250.0
    base4 = run_start(r["exe"], P, state[4:5], coeffs[4:5], o, COLD, starts[4:5])
    got = run_start(r["exe"], P, state, coeffs, o, modes, starts)
    np.testing.assert_array_equal(got["used"], [-1, -1, -1, PRIMAL, -2, FULL, FULL, PRIMAL])
    same_bits(got, r["ncold"], rows=slice(0, 3))
    for k in ("status", "iters", "diag", "obj", "u0", "traj", "sol"):
        np.testing.assert_array_equal(got[k][4], base4[k][0], err_msg=k)
    # the other rows of the batch are unaffected
    same_bits(got, base, rows=[3, 5, 6, 7])


# ---------------------------------------------------------------- 5. refusals without a GPU
def test_solve_start_refuses_null_start_before_the_handle(libmpcg):
    L = libmpcg
    one_d, one_i = (C.c_double * 8)(), (C.c_int32 * 2)()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    host = (L.mpcg_solve_start, 16, C.cast(one_d, dp), C.cast(one_i, ip))
    devc = (L.mpcg_solve_device_start, 17, C.c_void_p(C.addressof(one_d)), C.c_void_p(C.addressof(one_i)))
    for fn, nargs, start, mode in (host, devc):
        args = [None, 1] + [None] * (nargs - 2)
        assert fn(*args) == -1
        assert b"start and start_mode are required" in L.mpcg_last_error()
        args[5] = start
        assert fn(*args) == -1
        assert b"start and start_mode are required" in L.mpcg_last_error()
        # a start and a mode, no handle: the handle's refusal
        args[6] = mode
        assert fn(*args) == -1
        assert b"null handle" in L.mpcg_last_error()
    assert L.mpcg_abi_version() == 2
