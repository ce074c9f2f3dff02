"""Generate the committed golden fixtures under tests/golden/.

Run in the development container (needs /root/reference for the CppAD part):

    python tests/golden/make_goldens.py

Fixtures (data only -- inputs and expected outputs):
  cppad_derivs.npz   f, g, grad f, J_g, Lagrangian Hessian of the reference NLP at
                     seeded points, computed by the reference's vendored CppAD
                     (oracle/ref_probe/cppad_fg.cpp -> oracle/_ref/cppad_fg)
  hs071.json         the reference's known answer (assets/document/example/CppAD_Ipopt.cpp:146-150)
  infinity_N20.npz   256 infinity-set problems + 32 edge cases, plugin defaults,
                     solved by the oracle (Ipopt restatement, Ipopt default options)
  variants.npz       other parameter sets (class defaults, W_DA = 0, rate penalty on w,
                     N = 40, N = 3, small BOUND with active state bounds, N = 80, N = 100)
  preprocess.npz     findBestPath inputs (poses, waypoints) and the oracle's outputs
  bicycle_N25.npz    the kinematic-bicycle variant (BASELINE configs[4]; no reference
                     implementation exists, so this pins the build's own restatement):
                     64 infinity-set problems, N = 25, MODEL = 1, LF = 0.5, ANGVEL = 0.5
  ipopt_features.npz problems of the infinity set on which Ipopt's second-order
                     corrections, watchdog, soft restoration and restoration phase act
                     (found by scanning with the oracle's diagnostics), the problems the
                     round-1 advisor named for the bounded filter (16101, 1887), and the
                     max_cpu_time iteration budget forced low; per problem the parameter
                     set (N20 / N40 / N65 / bicycle), the oracle's diagnostics and results

All solves use the reference's options (oracle.pyoracle.ref_opts: Ipopt 3.12 defaults,
max_cpu_time 0.5 s as its iteration budget).

    python tests/golden/make_goldens.py [set ...]     (default: all sets)

  option_cases.json  the option matrix of tests/test_option_matrix.py and tests/test_gpu_options.py:
                     per case the option or parameter overrides and the infinity-set rows it runs
                     on (names, numbers and indices only), chosen by a scan with the oracle --
                     rows on which the case acts and on which the oracle's status and iteration
                     count do not depend on its linear algebra; the same per kernel instance
                     shape, on the restoration sets, and the fp32 solver's rows.  Not part of "all sets" (about ten
                     minutes on 8 cores):

    python tests/golden/make_goldens.py option_cases

  general.npz        MPC::Solve's arguments away from the infinity course (any pose, speeds from
                     reversing to above REF_V, far-off errors and steep polynomials, exact lines and
                     the all-zero problem) at six shapes (N = 20, 40, 65, 3, the bicycle at N = 25, the
                     class defaults), seeded; a row is kept when the oracle's status and iteration
                     count do not depend on its linear algebra.  Not part of "all sets"; the same
                     bytes on every run:

    python tests/golden/make_goldens.py general
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle as O  # noqa: E402
from mpc_ros_amd import infinity, params  # noqa: E402

PLUGIN = params.PLUGIN_DEFAULTS


def cppad_derivs():
    probe = os.path.join(ROOT, "oracle", "_ref", "cppad_fg")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    rng = np.random.default_rng(7)
    out = {}
    for N, K in ((6, 8), (20, 2)):
        P = dict(PLUGIN, STEPS=N, W_DANGVEL=30.0)
        nx, ng = 8 * N - 2, 6 * N
        st, cf = infinity.make_problems(np.arange(100, 100 + K))
        X = rng.normal(scale=0.6, size=(K, nx))
        SIG = rng.uniform(0.2, 2.0, size=K)
        LAM = rng.normal(scale=50.0, size=(K, ng))
        hdr = (f"{N} {P['DT']} {P['REF_CTE']} {P['REF_ETHETA']} {P['REF_V']} {P['W_CTE']} {P['W_EPSI']} "
               f"{P['W_V']} {P['W_ANGVEL']} {P['W_A']} {P['W_DANGVEL']} {P['W_DA']}\n{K}\n")
        body = []
        for k in range(K):
            body.append(" ".join(repr(float(v)) for v in np.concatenate([cf[k], X[k], [SIG[k]], LAM[k]])))
        res = subprocess.run([probe], input=hdr + "\n".join(body) + "\n", capture_output=True, text=True,
                             check=True).stdout.split()
        vals = np.array(res, dtype=np.float64).reshape(K, -1)
        o = 0
        fg = vals[:, o:o + 1 + ng]; o += 1 + ng
        jac = vals[:, o:o + (1 + ng) * nx].reshape(K, 1 + ng, nx); o += (1 + ng) * nx
        hes = vals[:, o:o + nx * nx].reshape(K, nx, nx)
        out[f"N{N}_params"] = np.array([P[k] for k in params.KEYS])
        out[f"N{N}_coeffs"] = cf
        out[f"N{N}_x"] = X
        out[f"N{N}_sigma"] = SIG
        out[f"N{N}_lambda"] = LAM
        out[f"N{N}_fg"] = fg
        out[f"N{N}_jac"] = jac
        out[f"N{N}_hess"] = hes
    out["keys"] = np.array(params.KEYS)
    np.savez_compressed(os.path.join(HERE, "cppad_derivs.npz"), **out)


def solve_set(P, st, cf, opts=None):
    r = O.mpc_solve_batch(P, st, cf, opts=opts or O.ref_opts(int(P["STEPS"])), nthreads=os.cpu_count() or 8,
                          diag=True)
    # (the fixtures keep diag's first five columns; the oracle's later ones, the slack margins, are
    # checked on a live solve by tests/test_oracle.py)
    return dict(state=st, coeffs=cf, u0=r["u0"], traj=r["traj"], obj=r["obj"], status=r["status"],
                iters=r["iters"], diag=np.ascontiguousarray(r["diag"][:, :5]), params=np.array([P[k] for k in params.KEYS]))


def infinity_set():
    st, cf = infinity.make_problems(np.arange(256))
    est, ecf = infinity.problems_from_scenarios(infinity.edge_scenarios())
    st = np.concatenate([st, est])
    cf = np.concatenate([cf, ecf])
    d = solve_set(PLUGIN, st, cf)
    d["index"] = np.concatenate([np.arange(256), -1 - np.arange(32)])
    np.savez_compressed(os.path.join(HERE, "infinity_N20.npz"), **d)
    print("infinity_N20 status:", np.unique(d["status"], return_counts=True), "iters mean", d["iters"].mean())


VARIANTS = {
    "class_defaults": (params.CLASS_DEFAULTS, 64, 1000),
    "no_rate": (dict(PLUGIN, W_DA=0.0), 64, 2000),
    "rate_w": (dict(PLUGIN, W_DANGVEL=50.0), 32, 3000),
    "N40": (dict(PLUGIN, STEPS=40), 24, 4000),
    "N3": (dict(PLUGIN, STEPS=3), 16, 5000),
    "small_bound": (dict(PLUGIN, BOUND=0.4), 16, 6000),
    # the cfg's STEPS range reaches 100 (MPCPlanner.cfg:22): two stage blocks per wavefront
    "N80": (dict(PLUGIN, STEPS=80), 8, 8000),
    "N100": (dict(PLUGIN, STEPS=100), 8, 9000),
}


def variants():
    out = {}
    for name, (P, n, off) in VARIANTS.items():
        st, cf = infinity.make_problems(np.arange(off, off + n))
        d = solve_set(P, st, cf)
        for k, v in d.items():
            out[f"{name}__{k}"] = v
        print(name, "status:", np.unique(d["status"], return_counts=True), "iters mean", d["iters"].mean())
    out["keys"] = np.array(params.KEYS)
    np.savez_compressed(os.path.join(HERE, "variants.npz"), **out)


def preprocess():
    idx = np.arange(64)
    sc = infinity.draw_scenarios(idx)
    px, py, yaw, plan = infinity.scenario_poses(sc)
    st = np.zeros((len(idx), 6))
    cf = np.zeros((len(idx), 4))
    for b in range(len(idx)):
        rc, st[b], cf[b] = O.find_best_path(px[b], py[b], yaw[b], sc["v"][b], sc["w_prev"][b], sc["a_prev"][b],
                                            0.1, plan[b], True)
        assert rc == 0
    np.savez_compressed(os.path.join(HERE, "preprocess.npz"), pose=np.stack([px, py, yaw], 1),
                        vel=np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], 1), plan=plan, dt=0.1, state=st,
                        coeffs=cf)


BICYCLE = dict(PLUGIN, STEPS=25, MODEL=1, LF=0.5, ANGVEL=0.5)


def bicycle():
    st, cf = infinity.make_problems(np.arange(7000, 7064))
    d = solve_set(BICYCLE, st, cf)
    d["model"] = np.int32(1)
    d["lf"] = np.float64(BICYCLE["LF"])
    np.savez_compressed(os.path.join(HERE, "bicycle_N25.npz"), **d)
    print("bicycle_N25 status:", np.unique(d["status"], return_counts=True), "iters mean", d["iters"].mean())


FEATURE_SETS = {
    # name: (params, problem indices of the infinity set)
    # N20: second-order corrections (7, 11, 25, 932: different local minimum without them;
    # 2571: two corrections), soft restoration (5045, 8938), restoration phase (1443),
    # round-1 advisor's filter-size problems (1887, 16101)
    "N20": (PLUGIN, [7, 11, 25, 932, 2571, 5045, 8938, 1443, 1887, 16101]),
    # N40: watchdog (88: six activations, 460, 842, 2012, 2094), soft restoration (422, 429,
    # 1431), restoration phase (69, 1167, 1204, 2956, 3441)
    "N40": (dict(PLUGIN, STEPS=40), [88, 460, 842, 2012, 2094, 422, 429, 1431, 69, 1167, 1204, 2956, 3441]),
    # bicycle N25: watchdog (3308), soft restoration (1292), corrections (18, 23), restoration
    # phase (4330: 120 iterations, 4720)
    "bicycle": (BICYCLE, [3308, 1292, 18, 23, 4330, 4720]),
    # the feasibility-restoration phase (round 3, found by scanning problems 0..131071 at
    # N = 20 and 0..32767 at N = 40 with the oracle's diagnostics): every problem of those
    # ranges on which Ipopt enters it
    "resto_N20": (PLUGIN, [1443, 40852, 74511, 84582]),
    "resto_N40": (dict(PLUGIN, STEPS=40), [69, 1167, 1204, 2956, 3441, 4626, 8420, 9871, 18581, 18819, 19148,
                                            19304, 23287, 25150, 25384, 28303, 30285, 31014, 31746]),
    # the restoration phase at the smallest shape of two stage blocks per wavefront
    "resto_N65": (dict(PLUGIN, STEPS=65), [1581]),
}


def ipopt_features():
    out = {}
    for name, (P, idx) in FEATURE_SETS.items():
        st, cf = infinity.make_problems(np.array(idx))
        d = solve_set(P, st, cf)
        d["index"] = np.array(idx)
        for k, v in d.items():
            out[f"{name}__{k}"] = v
        print(name, "status", d["status"].tolist(), "iters", d["iters"].tolist())
        print("   diag (soc, watchdog, soft, resto, resto iters):", d["diag"].tolist())
    # the max_cpu_time budget forced low: 0.005 s -> ora_cpu_iter_budget iterations at N = 20
    P = PLUGIN
    st, cf = infinity.make_problems(np.arange(0, 32))
    budget = O.cpu_iter_budget(0.005, 20)
    d = solve_set(P, st, cf, opts=O.ref_opts(20, cpu_iter_budget=budget))
    for k, v in d.items():
        out[f"budget__{k}"] = v
    out["budget__max_cpu_time"] = np.float64(0.005)
    out["budget__iter_budget"] = np.int32(budget)
    print("budget", budget, "status", np.unique(d["status"], return_counts=True))
    out["keys"] = np.array(params.KEYS)
    np.savez_compressed(os.path.join(HERE, "ipopt_features.npz"), **out)


# ---------------------------------------------------------------- general.npz
# Problems away from the infinity course: MPC::Solve's arguments drawn over their domain instead of
# produced by the preprocessing of a robot near the lemniscate.  Per category the state ranges and
# the scale of each polynomial coefficient (uniform in +- the scale):
#   pose   x, y in [-2, 2], psi in [-1.5, 1.5] (the y row of the initial-state constraint, the
#          polynomial at x < 0 and |x| > 2)
#   speed  x = y = psi = 0, v from reversing to above REF_V
#   far    x = y = psi = 0, cte and epsi far off, steep polynomials (atan of a steep slope, the
#          objective scaling at a large start gradient)
#   line   x = y = psi = 0, c0 = cte, c2 = c3 = 0 exactly, c1 = 0 on the even rows and uniform in
#          +- 0.5 on the odd ones; the first min(8, rows / 2) rows of a shape are the all-zero
#          problem, the even ones of them with v = REF_V (the start point is the optimum)
GENERAL_SEED = 2024
GENERAL_CATEGORIES = {
    # name: (x, y, psi half-ranges, v range, cte half-range, epsi half-range, coefficient scales)
    "pose": ((2.0, 2.0, 1.5), (0.0, 0.8), 0.5, 1.0, (0.5, 0.6, 0.2, 0.05)),
    "speed": ((0.0, 0.0, 0.0), (-0.6, 1.5), 0.3, 0.5, (0.3, 0.4, 0.1, 0.03)),
    "far": ((0.0, 0.0, 0.0), (0.0, 0.8), 2.5, 3.0, (2.5, 3.0, 1.0, 0.5)),
    "line": ((0.0, 0.0, 0.0), (0.0, 0.8), 0.4, 0.8, (0.0, 0.5, 0.0, 0.0)),
}
GENERAL_SHAPES = {
    # name: (params, rows per category); BOUND is the parameter set's own
    "N20": (PLUGIN, 16),
    "N40": (dict(PLUGIN, STEPS=40), 4),
    "N65": (dict(PLUGIN, STEPS=65), 2),
    "bicycle_N25": (BICYCLE, 4),
    "class_defaults": (params.CLASS_DEFAULTS, 4),
    "N3": (dict(PLUGIN, STEPS=3), 2),
}
GENERAL_MIN_KEPT = 0.95


def general_draw(shape, cat):
    """(state, coeffs) of a shape's rows of a category: a pure function of GENERAL_SEED and the two
    names' positions in the tables above."""
    P, n = GENERAL_SHAPES[shape]
    pose, (v0, v1), cte, eps, scale = GENERAL_CATEGORIES[cat]
    rng = np.random.default_rng([GENERAL_SEED, list(GENERAL_SHAPES).index(shape), list(GENERAL_CATEGORIES).index(cat)])
    st = np.zeros((n, 6))
    st[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) * np.array(pose)
    st[:, 3] = rng.uniform(v0, v1, n)
    st[:, 4] = rng.uniform(-cte, cte, n)
    st[:, 5] = rng.uniform(-eps, eps, n)
    cf = rng.uniform(-1.0, 1.0, (n, 4)) * np.array(scale)
    if cat == "line":
        cf[:, 0] = st[:, 4]
        cf[::2, 1] = 0.0
        nz = min(8, n // 2)
        st[:nz], cf[:nz] = 0.0, 0.0
        st[:nz:2, 3] = P["REF_V"]
    return st + 0.0, cf + 0.0  # (no negative zeros)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)


def general():
    """tests/golden/general.npz.  A drawn row is kept when the oracle's status and iteration count
    are the same with the dense solve, the structured solve and one refinement step, and the
    iteration count is at most MAX_ROW_ITERS; nothing else drops a row (no solver of the project
    is run here)."""
    out = {}
    for shape, (P, n) in GENERAL_SHAPES.items():
        N = int(P["STEPS"])
        draws = [general_draw(shape, cat) for cat in GENERAL_CATEGORIES]
        st, cf = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
        cat = np.repeat(np.array(list(GENERAL_CATEGORIES)), n)
        d = solve_set(P, st, cf)
        keep = d["iters"] <= MAX_ROW_ITERS
        for kw in (dict(kkt_structured=1), dict(refine_steps=1)):
            v = O.mpc_solve_batch(P, st, cf, opts=O.ref_opts(N, **kw), nthreads=os.cpu_count() or 8)
            keep &= (v["status"] == d["status"]) & (v["iters"] == d["iters"])
        print(f"general {shape}: kept {keep.sum()} of {len(keep)} ({100.0 * keep.mean():.1f} %), status",
              np.unique(d["status"][keep], return_counts=True), "iters max", d["iters"][keep].max())
        if keep.mean() < GENERAL_MIN_KEPT:
            raise SystemExit(f"general {shape}: fewer than {100 * GENERAL_MIN_KEPT:.0f} % of the rows kept")
        for c in GENERAL_CATEGORIES:
            if not keep[cat == c].any():
                raise SystemExit(f"general {shape}: no row of category {c} kept")
        for k, v in d.items():
            out[f"{shape}__{k}"] = v if k == "params" else v[keep]
        out[f"{shape}__category"] = cat[keep]
        if "MODEL" in P:
            out[f"{shape}__model"] = np.int32(P["MODEL"])
            out[f"{shape}__lf"] = np.float64(P["LF"])
    out["keys"] = np.array(params.KEYS)
    write_npz(os.path.join(HERE, "general.npz"), out)


def hs071():
    with open(os.path.join(HERE, "hs071.json"), "w") as f:
        json.dump({"source": "assets/document/example/CppAD_Ipopt.cpp:146-150",
                   "x": [1.000000, 4.743000, 3.82115, 1.379408], "zl": [1.087871, 0.0, 0.0, 0.0],
                   "zu": [0.0, 0.0, 0.0, 0.0], "rel_tol": 1e-6, "abs_tol": 1e-6}, f, indent=1)


# ---------------------------------------------------------------- option_cases.json
# name: (mpcg_params option fields, reference keys[, keys kept in the comparison's baseline
# [, options kept in it: the options that enable the one the case is about]])
ACC = dict(acceptable_tol=1e-3, acceptable_iter=3)
ACC2 = dict(acceptable_tol=1e-2, acceptable_iter=2)
OPTION_CASES = {
    "tol_1e-5": (dict(tol=1e-5), {}),
    "tol_1e-10": (dict(tol=1e-10), {}),
    "max_iter_7": (dict(max_iter=7), {}),
    "max_iter_0": (dict(max_iter=0), {}),
    "mu_init_1": (dict(mu_init=1.0), {}),
    "mu_init_1e-3": (dict(mu_init=1e-3), {}),
    "bound_relax_1e-4": (dict(bound_relax_factor=1e-4), {}),
    "acceptable_iter_2": (dict(ACC2), {}),
    "acceptable_tol_1e-3": (dict(ACC), {}),
    "acceptable_obj_change": (dict(ACC, acceptable_obj_change_tol=1e-6), {}, {}, ACC),
    "acceptable_constr_viol": (dict(ACC, acceptable_constr_viol_tol=1e-9), {}, {}, ACC),
    "acceptable_dual_inf": (dict(ACC2, acceptable_dual_inf_tol=1e-4), {}, {}, ACC2),
    "acceptable_compl_inf": (dict(ACC2, acceptable_compl_inf_tol=1e-7), {}, {}, ACC2),
    "kappa_soc_0.5": (dict(kappa_soc=0.5), {}),
    "max_soc_1": (dict(max_soc=1), {}),
    "watchdog_trigger_3": (dict(watchdog_shortened_iter_trigger=3), {}),
    "watchdog_trial_max_1": (dict(watchdog_trial_iter_max=1), {}),
    "soft_resto_factor_0": (dict(soft_resto_pderror_reduction_factor=0.0), {}),
    "soft_resto_factor_0.5": (dict(soft_resto_pderror_reduction_factor=0.5), {}),
    "max_soft_resto_iters_1": (dict(max_soft_resto_iters=1), {}),
    "obj_max_inc_0.5": (dict(obj_max_inc=0.5), {}),
    "max_filter_resets_0": (dict(max_filter_resets=0), {}),
    "filter_reset_trigger_1": (dict(filter_reset_trigger=1), {}),
    "filter_reset_trigger_2": (dict(filter_reset_trigger=2, max_filter_resets=1), {}),
    "tiny_step": (dict(tiny_step_tol=1e-4, tiny_step_y_tol=1e3), {}),
    "dual_inf_tol_1e-9": (dict(dual_inf_tol=1e-9), {}),
    "constr_viol_tol_1e-12": (dict(constr_viol_tol=1e-12), {}),
    # (below tol: the barrier parameter's floor follows it, tests/test_option_matrix.py's docstring)
    "compl_inf_tol_1e-9": (dict(compl_inf_tol=1e-9), {}),
    "no_restoration": (dict(no_restoration=1), {}),
    "max_cpu_time": (dict(max_cpu_time=0.005), {}),
    "ref_cte": ({}, dict(REF_CTE=0.3)),
    "ref_etheta": ({}, dict(REF_ETHETA=0.2)),
    "ref_negative": ({}, dict(REF_CTE=-0.3, REF_ETHETA=-0.2)),
    "dt_0.05": ({}, dict(DT=0.05)),
    "dt_0.25": ({}, dict(DT=0.25)),
    "ref_v": ({}, dict(REF_V=0.3)),
    "w_v_0": ({}, dict(W_V=0.0)),
    "w_cte_0": ({}, dict(W_CTE=0.0)),
    "w_epsi_0": ({}, dict(W_EPSI=0.0)),
    "w_angvel_w_a_0": ({}, dict(W_ANGVEL=0.0, W_A=0.0)),
    "w_dangvel_7": ({}, dict(W_DANGVEL=7.0, W_DA=0.0)),
    "w_da_7": ({}, dict(W_DANGVEL=0.0, W_DA=7.0)),
    "maxthr": ({}, dict(MAXTHR=0.3)),
    "angvel": ({}, dict(ANGVEL=0.2)),
    "angvel_maxthr": ({}, dict(ANGVEL=0.2, MAXTHR=2.5)),
    "bound_3": ({}, dict(BOUND=3.0)),
    "bound_1e6": ({}, dict(BOUND=1e6)),
    "model_bicycle": ({}, dict(MODEL=1, LF=0.5, ANGVEL=0.5)),
    "lf_0.2": ({}, dict(LF=0.2), dict(MODEL=1, LF=0.5)),
    "lf_2": ({}, dict(LF=2.0, REF_ETHETA=0.1, DT=0.05), dict(MODEL=1, LF=0.5)),
    "steps_7": ({}, dict(STEPS=7, REF_CTE=0.3, DT=0.2)),
}
# the cases tests/test_gpu_options.py runs across the kernel's instance shapes, and the shapes
SHAPE_CASES = ("max_iter_7", "mu_init_1", "acceptable_iter_2", "tiny_step", "bound_relax_1e-4", "filter_resets_off")
SHAPE_EXTRA = {"filter_resets_off": (dict(filter_reset_trigger=1, soft_resto_pderror_reduction_factor=0.0), {})}
SHAPES = {"N33": dict(STEPS=33), "N40": dict(STEPS=40), "N48": dict(STEPS=48), "N65": dict(STEPS=65),
          "bicycle_N25": dict(STEPS=25, MODEL=1, LF=0.5, ANGVEL=0.5),
          "bicycle_N33": dict(STEPS=33, MODEL=1, LF=0.5, ANGVEL=0.5),
          "bicycle_N40": dict(STEPS=40, MODEL=1, LF=0.5, ANGVEL=0.5),
          "bicycle_N48": dict(STEPS=48, MODEL=1, LF=0.5, ANGVEL=0.5)}
PARK_CANDIDATES = {"tol_1e-5": dict(tol=1e-5), "mu_init_1e-3": dict(mu_init=1e-3),
                   "watchdog_trigger_3": dict(watchdog_shortened_iter_trigger=3),
                   "filter_reset_trigger_1": dict(filter_reset_trigger=1), "dual_inf_tol_1e-9": dict(dual_inf_tol=1e-9)}
MAX_ROW_ITERS = 120
_BASELINES = {}


def _scan(case, idx, want=6, pad=2, total=4, need_status=(), max_iters=MAX_ROW_ITERS):
    """Rows of the infinity-set indices idx for a case: those on which the case acts (status,
    iteration count, or u0 by more than 1e-9 against the baseline) and on which the oracle's
    status and iteration count are the same with the dense solve, the structured solve and one
    refinement step; at most `want` of them (one of every ending first, then the shortest), plus
    `pad` well-conditioned rows on which it does not act (more, up to `total` rows in all).  The structured oracle (4x faster)
    screens, the dense oracle decides."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_option_matrix as T

    nt = os.cpu_count() or 8
    st, cf = infinity.make_problems(np.asarray(idx, dtype=np.int64))
    key = (json.dumps([T.case_params(case, baseline=True), case.get("baseline_options", {})], sort_keys=True), len(idx),
           int(np.asarray(idx).sum()))
    if key not in _BASELINES:  # (the defaults' results over a range: once)
        _BASELINES[key] = T.oracle_case(O, case, st, cf, baseline=True, threads=nt, kkt_structured=1)
    d = _BASELINES[key]
    r = T.oracle_case(O, case, st, cf, threads=nt, kkt_structured=1)
    act = T.acting_rows(r, d) & (r["iters"] <= max_iters)
    # candidates: every acting row (up to 32, rare endings first) and a few that do not act
    order = sorted(np.flatnonzero(act), key=lambda b: (r["status"][b] == 1, r["iters"][b]))[:32]
    cand = np.array(order + list(np.flatnonzero(~act & (r["iters"] <= max_iters))[:max(pad, total) + 2]), dtype=np.int64)
    if len(cand) == 0:
        return [], [], {}
    cst, ccf = st[cand], cf[cand]
    dd = T.oracle_case(O, case, cst, ccf, baseline=True, threads=nt)
    rr = T.oracle_case(O, case, cst, ccf, threads=nt)
    ok = np.ones(len(cand), bool)
    for kw in (dict(kkt_structured=1), dict(refine_steps=1)):
        v = T.oracle_case(O, case, cst, ccf, threads=nt, **kw)
        ok &= (v["status"] == rr["status"]) & (v["iters"] == rr["iters"])
    acts = T.acting_rows(rr, dd)
    good = [i for i in range(len(cand)) if ok[i] and acts[i]]
    chosen = []
    for s in list(need_status) + sorted(set(rr["status"][good].tolist())):  # one of every ending first
        for i in good:
            if rr["status"][i] == s and i not in chosen:
                chosen.append(i)
                break
    for i in sorted(good, key=lambda i: rr["iters"][i]):
        if len(chosen) >= want:
            break
        if i not in chosen:
            chosen.append(i)
    chosen = chosen[:want]
    quiet = [i for i in range(len(cand)) if ok[i] and not acts[i]][:max(pad, total - len(chosen))]
    info = dict(acting=len(good), status=sorted(set(rr["status"][chosen].tolist())),
                resto=int((rr["diag"][chosen + quiet, 3] > 0).sum()) if chosen + quiet else 0)
    return [int(np.asarray(idx)[cand[i]]) for i in chosen], [int(np.asarray(idx)[cand[i]]) for i in quiet], info


def _fp32_rows():
    """Rows of the two fixtures for the fp32 solver alone (tests/test_gpu_options.py), chosen with
    the host emulation's float solver (wide_host_check.cpp, HOST_T = float) under FP32_OPTIONS
    without restoration: 8 rows that need more than 5 iterations, on the infinity fixture four of
    them ended at an acceptable point by acceptable_iter 1 with acceptable_tol 1e-1."""
    import tempfile

    import test_core_host as H
    from conftest import load_npz, params_from_array

    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "whc32")
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-w", "-pthread", "-DHOST_T=float", "-o", exe,
                               os.path.join(ROOT, "tests", "native", "wide_host_check.cpp")])
        v, inf = load_npz("variants.npz"), load_npz("infinity_N20.npz")
        for name, par, st, cf in (("N40", v["N40__params"], v["N40__state"], v["N40__coeffs"]),
                                  ("infinity", inf["params"], inf["state"], inf["coeffs"])):
            P = params_from_array(par)
            res = {}
            for acc_iter in (15, 1):
                o = H.fp32_opts(O, P["STEPS"])
                o.restoration, o.acceptable_iter = 0, acc_iter
                if acc_iter == 1:
                    o.acceptable_tol = 1e-1
                res[acc_iter] = H.run_harness(exe, P, st, cf, opts=o)
            long_ = res[15]["iters"] > 5
            acc = np.flatnonzero(long_ & (res[1]["status"] == 4))[:4].tolist()
            rest = [int(b) for b in np.flatnonzero(long_ & (res[1]["status"] != 4)) if b not in acc][:8 - len(acc)]
            out[name] = dict(rows=sorted(rest + acc), acceptable=len(acc))
            print("fp32", name, out[name], flush=True)
    return out


def option_cases():
    """tests/golden/option_cases.json, all of it: for every case of OPTION_CASES the rows it runs
    on, found with the oracle over growing ranges of the infinity set (the features sets' indices
    and 0..255 first, then 0..8191, then 0..65535; a case without an acting row in all of them and
    in the features sets at N = 40 is recorded inert); the same per kernel instance shape; the
    restoration sets' rows for options across a park; the fp32 solver's rows."""
    path = os.path.join(HERE, "option_cases.json")
    if not os.path.exists(path):  # (tests/test_option_matrix.py, whose helpers the scan uses, reads it)
        with open(path, "w") as f:
            json.dump(dict(cases=[], shapes={}, park={}, fp32={}), f)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    feat20 = FEATURE_SETS["N20"][1] + FEATURE_SETS["resto_N20"][1]
    feat40 = FEATURE_SETS["N40"][1] + FEATURE_SETS["resto_N40"][1]
    cases = []
    for name, spec in OPTION_CASES.items():
        opts, par = spec[0], spec[1]
        case = dict(name=name, options=opts, params=par)
        if len(spec) > 2 and spec[2]:
            case["baseline_params"] = spec[2]
        if len(spec) > 3:
            case["baseline_options"] = spec[3]
        pools = [sorted(set(feat20) | set(range(256))), np.arange(8192), np.arange(65536)]
        rows, quiet, info = [], [], {}
        for pool in pools:  # (a larger range while fewer than three rows act)
            found = _scan(case, pool)
            if len(found[0]) > len(rows):
                rows, quiet, info = found
            if len(rows) >= 3:
                break
        if not rows and "STEPS" not in par:  # the features sets at N = 40 (watchdog, soft restoration)
            c40 = dict(case, params=dict(par, STEPS=40), baseline_params=dict(case.get("baseline_params", {}), STEPS=40))
            rows, quiet, info = _scan(c40, feat40)
            if rows:
                case = c40
        if rows:
            case["rows"] = {"infinity": rows + quiet}
        else:
            case["inert"] = True
            case["scanned"] = "infinity 0..65535, features N20, features N40"
            case["rows"] = {"infinity": feat20[:8]}
        print(name, case["rows"], info, flush=True)
        cases.append(case)
    out = dict(cases=cases)
    # the same scan per instance shape (rows 0..1023 of the infinity set, 6 rows each)
    shapes = {}
    for sname, par in SHAPES.items():
        for cname in SHAPE_CASES:
            opts = (OPTION_CASES.get(cname) or SHAPE_EXTRA[cname])[0]
            case = dict(name=f"{sname}/{cname}", options=opts, params=par, baseline_params=par)
            need = {"acceptable_iter_2": (4,), "tiny_step": (3,)}.get(cname, ())
            rows, quiet, info = _scan(case, np.arange(1024), want=5, pad=1, total=6, need_status=need)
            print(case["name"], rows, quiet, info, flush=True)
            shapes.setdefault(sname, {})[cname] = dict(options=opts, rows=(rows + quiet)[:6])
    out["shapes"] = dict(params=SHAPES, cases=shapes)
    # options across a park: per restoration set the rows on which the option acts (up to 4),
    # filled up to 4 with rows on which it does not; kept where the option acts on the set and at
    # least two of the rows still enter the restoration phase under it (a park area of one entry
    # then overflows)
    park = {}
    for cname, opts in PARK_CANDIDATES.items():
        for sname in ("resto_N20", "resto_N40"):
            P, idx = FEATURE_SETS[sname]
            case = dict(name=f"{sname}/{cname}", options=opts, params=dict(STEPS=P["STEPS"]),
                        baseline_params=dict(STEPS=P["STEPS"]))
            rows, quiet, info = _scan(case, idx, want=4, pad=0, max_iters=400)
            print(case["name"], rows, quiet, info, flush=True)
            if rows and info.get("resto", 0) >= 2:
                park.setdefault(cname, {})[sname] = dict(rows=[idx.index(i) for i in rows + quiet], acting=len(rows),
                                                         resto=info["resto"])
    out["park"] = park
    out["fp32"] = _fp32_rows()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    O.build(force=True)
    if sys.argv[1:2] == ["option_cases"]:  # (not part of "all": a scan of several minutes)
        option_cases()
        sys.exit(0)
    if sys.argv[1:2] == ["general"]:  # (not part of "all": it is a pure function of its seed)
        general()
        sys.exit(0)
    sets = set(sys.argv[1:]) or {"hs071", "preprocess", "infinity", "variants", "bicycle", "features", "cppad"}
    if "hs071" in sets:
        hs071()
    if "preprocess" in sets:
        preprocess()
    if "infinity" in sets:
        infinity_set()
    if "variants" in sets:
        variants()
    if "bicycle" in sets:
        bicycle()
    if "features" in sets:
        ipopt_features()
    if "cppad" in sets:
        if os.path.isdir("/root/reference/mpc_ros/include/cppad"):
            cppad_derivs()
        else:
            print("reference tree absent: cppad_derivs.npz not regenerated")
