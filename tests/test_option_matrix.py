"""Every solver option and problem parameter against the oracle, on the CPU (no GPU needed).

tests/golden/option_cases.json is a table of cases: one Ipopt option of mpcg_params (or one
coupled group, such as acceptable_iter with acceptable_tol) or one group of reference keys
changed from the plugin's defaults, and the rows it runs on -- indices of the infinity set
(mpc_ros_amd/infinity.py), chosen by tests/golden/make_goldens.py option_cases() with the
oracle: rows on which the change acts and on which the oracle's own path does not depend on
its linear algebra.  For every case the host emulation of the device core
(tests/native/wide_host_check.cpp) must follow the oracle under the case iterate for iterate.
tests/test_gpu_options.py runs the same table through the C-ABI on the device.

compl_inf_tol below tol: Ipopt's MonotoneMuUpdate poses compl_inf_tol to the scaled problem
(apply_obj_scaling) before it takes the barrier parameter's floor, mu_min = min(tol, objective
scaling x compl_inf_tol) / 11.  Oracle and core once took min(tol, compl_inf_tol) / 11: where
the objective scaling (100 / max |grad f| <= 1) is small, that floor could not meet a
compl_inf_tol <= ~3e-8 on the unscaled complementarity, and a converged row iterated at the
floor until the tiny-step rule ended it with status 3 at an iteration set by rounding (at 1e-8
and 1e-9, 62 of the infinity set's first 96 rows, the oracle's dense, structured and refined
solves disagreeing on 7 and 5 of them).  With the scaled floor all 96 rows end with status 1
after at most 49 iterations under all three solves, and the table tests compl_inf_tol at 1e-9.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_core_host import FILTER_PEAKS, compare, run_harness, wide_harness  # noqa: F401

TABLE = json.load(open(os.path.join(GOLDEN, "option_cases.json")))
CASES = {c["name"]: c for c in TABLE["cases"]}
MAX_INERT = 3
# an inert case must have been scanned over at least this range before it is declared inert
INERT_RANGE = "infinity 0..65535, features N20, features N40"


def case_params(case, baseline=False):
    """The case's parameter map: the plugin's defaults with the case's reference keys.
    baseline: the map the case is compared with to show that it acts (the plugin's defaults;
    "baseline_params" keeps the keys a case needs on both sides, e.g. MODEL for an LF case, and
    "baseline_options" the options that enable the one the case is about)."""
    from mpc_ros_amd import params

    P = dict(params.PLUGIN_DEFAULTS)
    P.update(case.get("baseline_params", {}))
    if not baseline:
        P.update(case["params"])
    P["STEPS"] = int(P["STEPS"])
    if "MODEL" in P:
        P["MODEL"] = int(P["MODEL"])
    return P


def oracle_opts(O, N, options, **kw):
    """An oracle IpmOpts from mpcg_params option fields (the reference's options otherwise)."""
    o = O.ref_opts(int(N), **kw)
    for k, v in options.items():
        if k == "no_restoration":
            o.restoration = 0 if v else 1
        elif k == "max_cpu_time":
            o.cpu_iter_budget = O.cpu_iter_budget(v, int(N))
        elif k in ("filter_cap", "precision"):
            pass  # (not solver options of the oracle: its filter is unbounded, it runs in double)
        else:
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
    return o


def case_problems(case, features=None):
    """(state, coeffs) of the case's rows: infinity-set indices, or rows of a fixture set."""
    from mpc_ros_amd import infinity

    rows = case["rows"]
    if "infinity" in rows:
        return infinity.make_problems(np.asarray(rows["infinity"], dtype=np.int64))
    g = features[rows["set"]]
    sel = np.asarray(rows["rows"])
    return g["state"][sel], g["coeffs"][sel]


def oracle_case(O, case, st, cf, baseline=False, threads=8, **kw):
    P = case_params(case, baseline)
    o = oracle_opts(O, P["STEPS"], case.get("baseline_options", {}) if baseline else case["options"], **kw)
    return O.mpc_solve_batch(P, st, cf, opts=o, nthreads=threads, diag=True)


def acting_rows(r, d):
    """Rows on which a case's result r differs from the defaults' d: status, iteration count,
    or u0 by more than 1e-9."""
    return (r["status"] != d["status"]) | (r["iters"] != d["iters"]) | (np.abs(r["u0"] - d["u0"]).max(1) > 1e-9)


_oracle_results = {}


@pytest.fixture(scope="module")
def case_results(oracle, features_golden):
    """The oracle under each case (computed once per case, shared by the tests below)."""
    def get(name):
        if name not in _oracle_results:
            case = CASES[name]
            st, cf = case_problems(case, features_golden)
            _oracle_results[name] = (st, cf, oracle_case(oracle, case, st, cf))
        return _oracle_results[name]
    return get


def test_table_covers_every_option_and_key():
    """Every Ipopt option field of mpcg_params and every reference key appears in a case; 4 to
    12 rows each; at most MAX_INERT inert cases, each with the range that was scanned."""
    from mpc_ros_amd import _lib
    from mpc_ros_amd.params import KEYS

    problem_fields = {"steps", "model", "dt", "ref_cte", "ref_etheta", "ref_v", "w_cte", "w_etheta", "w_v", "w_angvel",
                      "w_accel", "w_angvel_d", "w_accel_d", "max_angvel", "max_throttle", "bound", "wheelbase"}
    # (filter_cap: test_filter_cap_does_not_change_results; precision: tests/test_gpu_fp32.py and
    # tests/test_gpu_options.py -- the oracle has neither)
    option_fields = {f for f, _ in _lib.MpcgParams._fields_} - problem_fields - {"filter_cap", "precision"}
    acting = [c for c in TABLE["cases"] if not c.get("inert")]
    inert = [c for c in TABLE["cases"] if c.get("inert")]
    seen_opts = set().union(*(c["options"].keys() for c in acting))
    seen_keys = set().union(*(c["params"].keys() for c in acting))
    inert_opts = set().union(*(c["options"].keys() for c in inert)) if inert else set()
    inert_keys = set().union(*(c["params"].keys() for c in inert)) if inert else set()
    assert option_fields <= seen_opts | inert_opts, option_fields - seen_opts - inert_opts
    assert set(KEYS) | {"MODEL", "LF"} <= seen_keys | inert_keys, set(KEYS) - seen_keys - inert_keys
    assert len(inert) <= MAX_INERT
    for c in inert:
        assert c["scanned"] == INERT_RANGE, c["name"]
    for c in TABLE["cases"]:
        n = len(c["rows"].get("infinity", c["rows"].get("rows")))
        assert 4 <= n <= 12, c["name"]
        assert len(c["options"]) + len(c["params"]) >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_case_acts_and_is_well_conditioned(oracle, case_results, name):
    """The change acts on at least one of the case's rows (an inert case: on none, bitwise) --
    against the reference's options, or for an option that only works inside a group against the
    group's enabling options ("baseline_options": acceptable_compl_inf_tol 1e-7 undoes what
    acceptable_iter 2 with acceptable_tol 1e-2 does, and so equals the defaults again) -- and
    the oracle's status and iteration count on every row are the same with its structured KKT
    solve and with one step of iterative refinement
    (test_oracle.py::test_small_bound_iteration_counts_depend_on_the_linear_algebra's criterion)."""
    case = CASES[name]
    st, cf, r = case_results(name)
    d = oracle_case(oracle, case, st, cf, baseline=True)
    if case.get("inert"):
        for k in ("status", "iters", "u0", "traj", "obj"):
            np.testing.assert_array_equal(r[k], d[k])
    else:
        assert acting_rows(r, d).any()
    for kw in (dict(kkt_structured=1), dict(refine_steps=1)):
        v = oracle_case(oracle, case, st, cf, **kw)
        np.testing.assert_array_equal(v["status"], r["status"])
        np.testing.assert_array_equal(v["iters"], r["iters"])


@pytest.mark.parametrize("name", list(CASES))
def test_wide_core_matches_oracle_under_case(wide_harness, oracle, case_results, name):  # noqa: F811
    case = CASES[name]
    st, cf, g = case_results(name)
    P = case_params(case)
    r = run_harness(wide_harness, P, st, cf, opts=oracle_opts(oracle, P["STEPS"], case["options"]))
    compare(r, g, atol=1e-7 if g["iters"].max() > 150 else 1e-9)


def test_status_coverage(case_results):
    """Success, the iteration limit, a tiny step, an acceptable point and local infeasibility
    each end some row of the table in the oracle."""
    seen = set()
    for name in CASES:
        seen |= set(case_results(name)[2]["status"].tolist())
    assert {1, 2, 3, 4, 5} <= seen, seen


def test_filter_cap_does_not_change_results(wide_harness, features_golden):  # noqa: F811
    """Results do not depend on filter_cap while fewer than filter_cap + 448 entries are held:
    the filter's LDS part of 1, 8, 63, 65 or 128 entries against 64, bitwise in every output,
    on the rows whose filters peak at 53, 51 and 196 entries; nothing dropped."""
    from concurrent.futures import ThreadPoolExecutor

    caps = (64, 1, 8, 63, 65, 128)
    jobs = []
    with ThreadPoolExecutor(len(caps) * len(FILTER_PEAKS)) as pool:  # (one harness process each)
        for name, peaks in FILTER_PEAKS.items():
            g = features_golden[name]
            rows = [int(np.flatnonzero(g["index"] == pid)[0]) for pid in peaks]
            for cap in caps:
                jobs.append((name, cap, pool.submit(run_harness, wide_harness, g["P"], g["state"][rows],
                                                    g["coeffs"][rows], filter_cap=cap)))
    res = {(name, cap): f.result() for name, cap, f in jobs}
    for name, peaks in FILTER_PEAKS.items():
        ref = res[name, 64]
        np.testing.assert_array_equal(ref["nf_peak"], list(peaks.values()))
        for cap in caps[1:]:
            r = res[name, cap]
            for k in ref:
                np.testing.assert_array_equal(r[k], ref[k], err_msg=f"{name} filter_cap {cap} {k}")
            assert (r["n_fover"] == 0).all()
