"""Per-problem parameter rows, host side (no GPU): the row layout of include/mpcg.h
(MPCG_PP_*), mpcg_pparams_fill / mpcg_pparams_check, params.rows, Tracking::deceleration's rule
(mpcg_decelerate) and the per-problem launch plan (tests/native/wide_plan_check.cpp).

Also the parameter recipe the GPU tests (tests/test_gpu_pparams.py) share: rows that differ from
each other and from the handle in every per-problem field.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from host_harness import build

PHI = 0.6180339887498949
WEIGHTS = ("W_CTE", "W_EPSI", "W_V", "W_ANGVEL", "W_A", "W_DANGVEL", "W_DA")


def u(i: int, k: int) -> float:
    return float(np.modf((i + 1) * PHI * (k + 1))[0])


def recipe(P: dict, i: int, vary_lf: bool = False) -> dict:
    """Row i's parameters from the set P: REF_V in [0.05, 1], the weights x [0.25, 4], the limits
    x [0.5, 1.5], the error references within +-0.1; BOUND, DT (and LF unless vary_lf) are P's."""
    d = dict(P)
    d["REF_V"] = 0.05 + 0.95 * u(i, 0)
    for j, k in enumerate(WEIGHTS):
        d[k] = P[k] * (0.25 + 3.75 * u(i, 1 + j))
    d["ANGVEL"] = P["ANGVEL"] * (0.5 + u(i, 8))
    d["MAXTHR"] = P["MAXTHR"] * (0.5 + u(i, 9))
    d["REF_CTE"] = 0.2 * (u(i, 10) - 0.5)
    d["REF_ETHETA"] = 0.2 * (u(i, 11) - 0.5)
    if vary_lf:
        d["LF"] = 0.5 * (0.8 + 0.4 * u(i, 12))
    return d


def other_handle_params(P: dict) -> dict:
    """The set P with every per-problem field changed: what the handle is created with, so a
    path that reads the handle instead of the row fails on values."""
    d = dict(P)
    d["REF_V"] = P["REF_V"] * 0.37
    for k in WEIGHTS:
        d[k] = P[k] * 2 + 1.0
    d["ANGVEL"] = P["ANGVEL"] * 0.5
    d["MAXTHR"] = P["MAXTHR"] * 0.8
    d["BOUND"] = P["BOUND"] * 0.5
    d["DT"] = P["DT"] * 1.5
    d["REF_CTE"], d["REF_ETHETA"] = 0.05, -0.05
    d["LF"] = P.get("LF", 0.5) * 1.3
    return d


def header_indices() -> dict:
    text = open(os.path.join(ROOT, "include", "mpcg.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define MPCG_PP_([A-Z_]+) (\d+)", text)}


# mpcg_params field of each row key
FIELD = {"DT": "dt", "REF_CTE": "ref_cte", "REF_ETHETA": "ref_etheta", "REF_V": "ref_v", "W_CTE": "w_cte",
         "W_EPSI": "w_etheta", "W_V": "w_v", "W_ANGVEL": "w_angvel", "W_A": "w_accel", "W_DANGVEL": "w_angvel_d",
         "W_DA": "w_accel_d", "ANGVEL": "max_angvel", "MAXTHR": "max_throttle", "BOUND": "bound", "LF": "wheelbase"}


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_row_layout_and_fill(libmpcg):
    """The header's indices are 0..15 in the stated order, params.ROW_KEYS is that order, and
    mpcg_pparams_fill writes each field of the set at its index (the reserved one 0)."""
    from mpc_ros_amd import _lib, params

    idx = header_indices()
    assert idx.pop("FIELDS") == 16 == _lib.PP_FIELDS == params.ROW_FIELDS
    assert idx.pop("RESERVED") == 15
    order = ("DT", "REF_CTE", "REF_ETHETA", "REF_V", "W_CTE", "W_EPSI", "W_V", "W_ANGVEL", "W_A", "W_DANGVEL", "W_DA",
             "ANGVEL", "MAXTHR", "BOUND", "LF")
    assert idx == {k: i for i, k in enumerate(order)} and params.ROW_KEYS == order
    p = _lib.MpcgParams()
    assert libmpcg.mpcg_params_plugin_default(C.byref(p)) == 0
    for i, k in enumerate(order):  # (a distinct value per field)
        setattr(p, FIELD[k], 0.5 + i)
    rows = np.full((3, 16), -7.0)
    assert libmpcg.mpcg_pparams_fill(C.byref(p), 3, _dp(rows)) == 0
    np.testing.assert_array_equal(rows, np.tile([0.5 + i for i in range(15)] + [0.0], (3, 1)))
    assert libmpcg.mpcg_pparams_fill(None, 3, _dp(rows)) < 0


def test_params_rows_against_fill(libmpcg):
    from mpc_ros_amd import _lib, params

    P = dict(params.PLUGIN_DEFAULTS, LF=0.4)
    dicts = [recipe(P, i, vary_lf=True) for i in range(5)]
    got = params.rows(dicts)
    assert got.shape == (5, 16) and got.dtype == np.float64
    for i, d in enumerate(dicts):
        p = _lib.params_from_map(d)
        want = np.zeros(16)
        assert libmpcg.mpcg_pparams_fill(C.byref(p), 1, _dp(want)) == 0
        np.testing.assert_array_equal(got[i], want)
    # a base dict and per-key arrays; STEPS and MODEL are not per-problem
    rv = np.array([0.1, 0.2, 0.3])
    b = params.rows(P, REF_V=rv, W_V=[1.0, 2.0, 3.0])
    assert b.shape == (3, 16)
    np.testing.assert_array_equal(b[:, 3], rv)
    np.testing.assert_array_equal(b[:, 6], [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(np.delete(b, [3, 6], axis=1), np.delete(params.rows([P] * 3), [3, 6], axis=1))
    np.testing.assert_array_equal(params.rows(P, B=2), params.rows([P, P]))
    assert params.rows({}, B=1)[0, 14] == 0.5  # (LF: the library's default wheelbase)
    with pytest.raises(KeyError):
        params.rows(P, STEPS=[20, 20])
    with pytest.raises(ValueError):
        params.rows(P, REF_V=[1.0, 2.0], W_V=[1.0])


# key: (value just outside its domain, the edge value inside), as test_abi.PARAM_DOMAIN
ROW_DOMAIN = {
    "DT": (0.0, 5e-324), "ANGVEL": (0.0, 5e-324), "MAXTHR": (0.0, 5e-324), "BOUND": (0.0, 5e-324),
    "W_CTE": (-5e-324, 0.0), "W_EPSI": (-5e-324, 0.0), "W_V": (-5e-324, 0.0), "W_ANGVEL": (-5e-324, 0.0),
    "W_A": (-5e-324, 0.0), "W_DANGVEL": (-5e-324, 0.0), "W_DA": (-5e-324, 0.0),
}


def _check(libmpcg, rows, model=0):
    bad = C.c_int64(-1)
    rc = libmpcg.mpcg_pparams_check(_dp(rows), rows.shape[0], model, C.byref(bad))
    return rc, bad.value


@pytest.mark.parametrize("key", list(ROW_DOMAIN))
def test_pparams_check_domain_edges(libmpcg, key):
    from mpc_ros_amd import params

    rows = params.rows(params.PLUGIN_DEFAULTS, B=6)
    assert _check(libmpcg, rows) == (0, -1)
    j = params.ROW_KEYS.index(key)
    outside, inside = ROW_DOMAIN[key]
    rows[4, j] = outside
    rc, bad = _check(libmpcg, rows)
    assert rc < 0 and bad == 4 and b"row 4" in libmpcg.mpcg_last_error()
    rows[4, j] = inside
    assert _check(libmpcg, rows) == (0, -1)


def test_pparams_check_finite_lf_and_first_bad_row(libmpcg):
    from mpc_ros_amd import params

    base = params.rows(params.PLUGIN_DEFAULTS, B=5)
    for j in range(15):  # every field read must be finite; the reserved one is not read
        for v in (np.nan, np.inf, -np.inf):
            rows = base.copy()
            rows[2, j] = v
            assert _check(libmpcg, rows)[0] < 0 and _check(libmpcg, rows)[1] == 2, (j, v)
    rows = base.copy()
    rows[:, 15] = np.nan
    assert _check(libmpcg, rows) == (0, -1)
    # LF > 0 for the bicycle only
    rows = base.copy()
    rows[1, 14] = 0.0
    assert _check(libmpcg, rows, model=0) == (0, -1)
    assert _check(libmpcg, rows, model=1) == (-1, 1)
    rows[1, 14] = 5e-324
    assert _check(libmpcg, rows, model=1) == (0, -1)
    # the first offending row is reported; a NULL bad_row is allowed
    rows = base.copy()
    rows[3, 6] = -1.0
    rows[1, 12] = 0.0
    assert _check(libmpcg, rows) == (-1, 1)
    assert libmpcg.mpcg_pparams_check(_dp(rows), 5, 0, None) < 0
    assert libmpcg.mpcg_pparams_check(_dp(rows), 5, 2, None) < 0  # (no such model)
    assert libmpcg.mpcg_pparams_check(_dp(rows), 0, 0, None) == 0


def decelerate_np(dist, v, max_throttle, max_speed, min_speed, ref_v):
    """Tracking::deceleration (driving_state.cpp:121-141) restated; returns (REF_V, outcome):
    0 unchanged, 1 max_speed, 2 min_speed, 3 speed."""
    dist, v, ref_v = np.broadcast_arrays(np.asarray(dist, float), np.asarray(v, float), np.asarray(ref_v, float))
    near = dist <= v * v / max_throttle
    speed = max_throttle * dist
    out = np.where(speed > ref_v, max_speed, np.where(speed < min_speed, min_speed, speed))
    kind = np.where(speed > ref_v, 1, np.where(speed < min_speed, 2, 3))
    return np.where(near, out, ref_v), np.where(near, kind, 0)


def test_decelerate_rule(libmpcg):
    """mpcg_decelerate over a grid that reaches all four outcomes, and the equalities at the
    branch edges: dist == v^2 / MAXTHR decelerates, speed == ref_v and speed == min_speed are
    `speed`."""
    thr, vmax, vmin = 0.8, 0.7, 0.05
    vs = np.array([0.0, 0.1, 0.3, 0.5, 0.8])
    dists = np.concatenate([np.linspace(0.0, 1.2, 25), vs * vs / thr, [vmin / thr, 0.5 / thr]])
    refs = np.array([0.04, 0.2, 0.5, 1.0])
    D, V, R = (a.ravel() for a in np.meshgrid(dists, vs, refs, indexing="ij"))
    want, kind = decelerate_np(D, V, thr, vmax, vmin, R)
    assert all((kind == k).sum() >= 10 for k in range(4)), np.bincount(kind)
    got = np.array([libmpcg.mpcg_decelerate(d, v, thr, vmax, vmin, r) for d, v, r in zip(D, V, R)])
    np.testing.assert_array_equal(got, want)
    f = libmpcg.mpcg_decelerate
    v = 0.5
    edge = v * v / thr
    assert f(edge, v, thr, vmax, vmin, 1.0) == thr * edge  # (<=: the edge decelerates)
    assert f(np.nextafter(edge, 1.0), v, thr, vmax, vmin, 1.0) == 1.0
    d = 0.25
    assert f(d, 0.8, thr, vmax, vmin, thr * d) == thr * d  # (speed == ref_v: not the max_speed branch)
    assert f(d, 0.8, thr, vmax, vmin, np.nextafter(thr * d, 0.0)) == vmax  # (the quirk: max_speed, not speed)
    assert f(vmin / thr, 0.8, thr, vmax, thr * (vmin / thr), 1.0) == thr * (vmin / thr)  # (speed == min_speed)
    assert f(0.01, 0.8, thr, vmax, vmin, 1.0) == vmin


def test_pp_plan_native_check():
    """tests/native/wide_plan_check.cpp (which checks every kind of instance): every pp_solve_key /
    pp_resume_key over model x N = 1..128 x default / non-default options x B in {1, 4096, 4097} is
    a row of the instance list under its kind, every row is chosen by some input, and fp32 is
    refused; with "pp" it prints the per-problem instance chosen under a non-default option."""
    exe = build("wide_plan_check", "-O1")
    r = subprocess.run([exe, "pp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "k_solve_wide_pp<0,true,double,1,false,2>" in r.stdout
