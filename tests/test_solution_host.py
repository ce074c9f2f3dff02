"""The solver's full solution record on the host (no GPU needed).

tests/native/wide_sol_check.cpp runs mpc_ros_amd/csrc/wide_core.h on 64 fibers and prints, after
the outputs every solve has, the record WideSolver::solution_out writes: x | z_L | z_U | lambda of
the original, unscaled NLP in the reference's variable and row order (include/mpcg.h).  It does
not compile without solution_out.

  * x is the oracle's full primal point (pyoracle.mpc_solve(full=True)) to 1e-7, the project's
    control tolerance, and bitwise the u0 / traj the same solve publishes;
  * z_L, z_U >= 0, and the three KKT residuals -- computed here in numpy from the oracle's
    function, gradient and dense Jacobian with the record's multipliers -- meet the Ipopt
    tolerances under which status 1 is returned (dual_inf_tol, constr_viol_tol, compl_inf_tol);
  * the dual residual is at most DUAL_RATIO_BOUND times the oracle's own final unscaled error
    of the same row: a wrong unscaling by the objective or a row scale must not hide under
    dual_inf_tol = 1.  DUAL_RATIO_MEASURED is the largest ratio over the fixture rows (printed by
    the test; DESIGN.md "The full solution and its certificate" explains what it consists of),
    the bound ten times it; the record with lambda multiplied by the row's objective scale
    (rows where it is below 0.5) fails the bound, so the bound does test the unscaling.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from conftest import load_npz, params_from_array
from host_harness import build, harness_stdin, opts_line

X_ATOL = 1e-7
# the largest dual residual / oracle kkt_inf over the status-1 rows of SETS, measured on the host
# emulation (test_multipliers_satisfy_kkt prints the figure of every set: 2.9e2 on the infinity rows,
# 6.5e2 on class_defaults, 3.151e3 on bicycle_N25 row 33), and the bound.  The residual is not the
# solver's own error (the oracle's kkt_inf, ~1e-8): x is published after honor_original_bounds, a
# variable at a relaxed bound moves by up to bound_relax_factor max(1, |bound|) while the
# multipliers stay, and the gradient moves with it -- 2 W_ANGVEL 3e-8 = 6e-6 at ANGVEL = 3, and
# through the bicycle's v delta / lf term |lambda| dt / lf 1e-8 = 3e-5.
# The general sets (problems away from the infinity course) are held to the same bound, which stays
# where the infinity-course rows put it: 2.9e2 on general_N20, 4.144e3 on general_bicycle_N25.
DUAL_RATIO_MEASURED = 3.151e3
DUAL_RATIO_BOUND = 10 * DUAL_RATIO_MEASURED

SETS = ["infinity", "variants_class_defaults", "variants_rate_w", "variants_no_rate", "variants_N40", "variants_N3",
        "variants_small_bound", "variants_N80", "variants_N100", "bicycle_N25", "resto_N20", "resto_N65",
        "general_N20", "general_bicycle_N25"]
# the shapes of tests/golden/general.npz (fixture_set("general_<shape>"))
GENERAL_SHAPES = ["N20", "N40", "N65", "bicycle_N25", "class_defaults", "N3"]


def fixture_set(name):
    """(parameter dict, golden arrays) of a set of SETS."""
    if name == "infinity":
        g = load_npz("infinity_N20.npz")
        return params_from_array(g["params"]), g
    if name == "bicycle_N25":
        g = load_npz("bicycle_N25.npz")
        P = params_from_array(g["params"])
        P.update(MODEL=int(g["model"]), LF=float(g["lf"]))
        return P, g
    if name.startswith("general_"):  # tests/golden/general.npz: problems away from the infinity course
        key = name[len("general_"):]
        g = {k.split("__", 1)[1]: v for k, v in load_npz("general.npz").items() if k.startswith(key + "__")}
        P = params_from_array(g["params"])
        if "model" in g:
            P.update(MODEL=int(g["model"]), LF=float(g["lf"]))
        return P, g
    fname, key = ("variants.npz", name[len("variants_"):]) if name.startswith("variants_") else ("ipopt_features.npz", name)
    z = load_npz(fname)
    g = {k.split("__", 1)[1]: v for k, v in z.items() if k.startswith(key + "__")}
    return params_from_array(g["params"]), g


def run_sol_harness(exe, P, state, coeffs, o):
    N = int(P["STEPS"])
    out = subprocess.run([exe], input=harness_stdin(P, state, coeffs, o, opts_line(o)), capture_output=True,
                         text=True, check=True).stdout
    rows = np.array([r.split() for r in out.strip().split("\n")], dtype=np.float64)
    assert rows.shape == (len(state), 5 + 3 * N + 3 * (8 * N - 2) + 6 * N)
    return dict(status=rows[:, 0].astype(int), iters=rows[:, 1].astype(int), obj=rows[:, 2], u0=rows[:, 3:5],
                traj=rows[:, 5:5 + 3 * N].reshape(len(state), 3, N), sol=np.ascontiguousarray(rows[:, 5 + 3 * N:]))


def split(sol, N):
    nx = 8 * N - 2
    return sol[..., :nx], sol[..., nx:2 * nx], sol[..., 2 * nx:3 * nx], sol[..., 3 * nx:]


def nlp_bounds(P, state):
    """MPC::Solve's original bounds: (xl, xu, g_bound) of one problem."""
    N = int(P["STEPS"])
    xu = np.r_[np.full(6 * N, P["BOUND"]), np.full(N - 1, P["ANGVEL"]), np.full(N - 1, P["MAXTHR"])]
    gb = np.zeros(6 * N)
    gb[::N] = state
    return -xu, xu, gb


def numpy_kkt(oracle, P, state, coeffs, sol):
    """The certificate of one record in numpy, from the oracle's fg, gradient and dense Jacobian:
    (stationarity, primal violation, complementarity, objective) and the magnitude
    max|grad f| + max|lambda| + max|z| the evaluation's rounding scales with."""
    N = int(P["STEPS"])
    x, zl, zu, lam = split(sol, N)
    fg = oracle.mpc_fg(P, coeffs, x)
    gf, J, _ = oracle.mpc_derivs(P, coeffs, x, 1.0, lam)
    xl, xu, gb = nlp_bounds(P, state)
    stat = np.abs(gf + J.T @ lam - zl + zu).max()
    prim = max(np.abs(fg[1:] - gb).max(), (xl - x).max(), (x - xu).max())
    comp = max(np.abs((x - xl) * zl).max(), np.abs((xu - x) * zu).max())
    scale = np.abs(gf).max() + np.abs(lam).max() + max(np.abs(zl).max(), np.abs(zu).max())
    return np.array([stat, prim, comp, fg[0]]), scale


def objective_scale(P, state):
    """The solver's (Ipopt's gradient-based) objective scaling of one problem: 100 / max|grad f|
    at the start point where that exceeds 100, else 1."""
    def gmax(s):
        return max(abs(2 * P["W_V"] * (s[3] - P["REF_V"])), abs(2 * P["W_CTE"] * (s[4] - P["REF_CTE"])),
                   abs(2 * P["W_EPSI"] * (s[5] - P["REF_ETHETA"])))
    gm = max(gmax(state), gmax(np.zeros(6)))
    return 100.0 / gm if gm > 100.0 else 1.0


_cache = {}


def records(name, oracle, tmp_path_factory):
    """Computed once per set and shared (tests/test_kkt_host.py too), never modified: the host
    emulation's outputs and records, the oracle's full solve of every row, the numpy certificate."""
    if name not in _cache:
        P, g = fixture_set(name)
        N = int(P["STEPS"])
        o = oracle.ref_opts(N)
        state, coeffs = np.ascontiguousarray(g["state"]), np.ascontiguousarray(g["coeffs"])
        r = run_sol_harness(build("wide_sol_check"), P, state, coeffs, o)
        ref = [oracle.mpc_solve(P, state[b], coeffs[b], opts=o, full=True) for b in range(len(state))]
        nk = [numpy_kkt(oracle, P, state[b], coeffs[b], r["sol"][b]) for b in range(len(state))]
        r.update(P=P, N=N, opts=o, state=state, coeffs=coeffs, ref_x=np.array([q["x"] for q in ref]),
                 ref_kkt=np.array([q["kkt"] for q in ref]), ref_status=np.array([q["status"] for q in ref]),
                 np_cert=np.array([c for c, _ in nk]), np_scale=np.array([s for _, s in nk]),
                 sf=np.array([objective_scale(P, s) for s in state]))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = r
    return _cache[name]


@pytest.fixture(params=SETS)
def rec(request, oracle, tmp_path_factory):
    return request.param, records(request.param, oracle, tmp_path_factory)


def test_x_is_the_oracles_point_and_the_published_one(rec):
    name, r = rec
    N = r["N"]
    x = split(r["sol"], N)[0]
    np.testing.assert_array_equal(r["status"], r["ref_status"])
    d = np.abs(x - r["ref_x"]).max()
    print(f"{name}: max |x - oracle x| = {d:.3e} over {len(x)} rows")
    assert d <= X_ATOL
    # bitwise the outputs of the same solve at the shared entries
    np.testing.assert_array_equal(x[:, :3 * N].reshape(-1, 3, N), r["traj"])
    np.testing.assert_array_equal(x[:, [6 * N, 7 * N - 1]], r["u0"])


def test_multipliers_satisfy_kkt(rec):
    name, r = rec
    N, o = r["N"], r["opts"]
    _, zl, zu, lam = split(r["sol"], N)
    assert (zl >= 0).all() and (zu >= 0).all() and np.isfinite(r["sol"]).all()
    ok = r["status"] == 1
    assert ok.any()
    c = r["np_cert"][ok]
    ratio = c[:, 0] / r["ref_kkt"][ok]
    print(f"{name}: {ok.sum()} status-1 rows: dual {c[:, 0].max():.3e} primal {c[:, 1].max():.3e} "
          f"compl {c[:, 2].max():.3e}; dual / oracle kkt_inf max {ratio.max():.3e}")
    # the conditions under which status 1 is returned
    assert c[:, 0].max() <= o.dual_inf_tol
    assert c[:, 1].max() <= o.constr_viol_tol
    assert c[:, 2].max() <= o.compl_inf_tol
    # the sharper bound on the unscaling
    assert ratio.max() <= DUAL_RATIO_BOUND


def test_general_set_sees_a_dropped_y_row(oracle, tmp_path_factory):
    """The general set's teeth: the certificate of a `pose` record under the same state with
    state[1] (y, 0 in every infinity problem) replaced by 0 reports the initial-state row of y as
    violated by |y0| -- a solver that dropped that row would not pass on this set."""
    r = records("general_N20", oracle, tmp_path_factory)
    _, g = fixture_set("general_N20")
    b = max(np.flatnonzero(g["category"] == "pose"), key=lambda i: abs(r["state"][i, 1]))
    y0 = r["state"][b, 1]
    assert abs(y0) >= 0.5 and r["status"][b] == 1
    assert r["np_cert"][b, 1] <= r["opts"].constr_viol_tol
    st = r["state"][b].copy()
    st[1] = 0.0
    c, _ = numpy_kkt(oracle, r["P"], st, r["coeffs"][b], r["sol"][b])
    print(f"general_N20 row {b}: y0 = {y0:.4f}, primal violation with y0 dropped {c[1]:.4f}")
    assert abs(c[1] - abs(y0)) <= 1e-6


def test_wrong_unscaling_fails_the_dual_bound(oracle, tmp_path_factory):
    """The negative control: lambda left in the scaled objective's units (times the objective
    scale) on the rows whose scale is below 0.5."""
    n = 0
    for name in SETS:
        r = records(name, oracle, tmp_path_factory)
        N = r["N"]
        for b in np.flatnonzero((r["status"] == 1) & (r["sf"] < 0.5)):
            sol = r["sol"][b].copy()
            split(sol, N)[3][:] *= r["sf"][b]
            c, _ = numpy_kkt(oracle, r["P"], r["state"][b], r["coeffs"][b], sol)
            assert c[0] / r["ref_kkt"][b] > DUAL_RATIO_BOUND, (name, b, c[0], r["ref_kkt"][b])
            n += 1
    print(f"{n} rows with an objective scale below 0.5")
    assert n >= 4
