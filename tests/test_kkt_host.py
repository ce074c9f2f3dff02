"""The KKT certificate on the host (no GPU needed): mpcg_kkt, the host loop over the stage body
the kernel k_kkt_certify runs per lane (mpc_ros_amd/csrc/mpcg_kkt.h), against the same residuals
computed in numpy from the oracle's function, gradient and dense Jacobian
(tests/test_solution_host.py numpy_kkt), on the records of the host emulation of the solver.

The tolerance of the comparison is pure re-evaluation -- sums of at most 16 terms in fp64 --
1e-11 (1 + max|grad f| + max|lambda| + max|z|) per row.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_solution_host import nlp_bounds, numpy_kkt, records, split

# both models, the split / unsplit / two-block horizons, rows through the restoration phase, and a
# set whose rows mostly end infeasible (the certificate reads any record, not only solutions)
# (general_*: records away from the infinity course -- y != 0, steep polynomials, exact lines)
KKT_SETS = ["infinity", "bicycle_N25", "variants_N40", "variants_N80", "variants_small_bound", "resto_N65",
            "general_N20", "general_bicycle_N25"]


def host_cert(libmpcg, r, sol=None, rows=None):
    from mpc_ros_amd import solver

    P = dict(r["P"])
    return solver.kkt(P, r["state"], r["coeffs"], r["sol"] if sol is None else sol, params_rows=rows)


def tol(r):
    return 1e-11 * (1 + r["np_scale"])


@pytest.mark.parametrize("name", KKT_SETS)
def test_host_mirror_equals_numpy(libmpcg, oracle, tmp_path_factory, name):
    r = records(name, oracle, tmp_path_factory)
    cert = host_cert(libmpcg, r)
    d = np.abs(cert[:, :3] - r["np_cert"][:, :3]).max(axis=1)
    print(f"{name}: max |mpcg_kkt - numpy| / tolerance = {(d / tol(r)).max():.3e}")
    assert (d <= tol(r)).all()
    # column 3 is the NLP's objective at the record's x: numpy's, and the solver's own obj
    np.testing.assert_allclose(cert[:, 3], r["np_cert"][:, 3], rtol=1e-12, atol=0)
    np.testing.assert_allclose(cert[:, 3], r["obj"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", ["infinity", "bicycle_N25"])
def test_perturbed_multiplier_raises_stationarity(libmpcg, oracle, tmp_path_factory, name):
    """lambda of the first initial-state row + 1e-3: that row's Jacobian is the unit vector of
    x_0, so the stationarity residual of x_0 moves by exactly 1e-3; the other columns do not read
    lambda."""
    r = records(name, oracle, tmp_path_factory)
    N, nx = r["N"], 8 * r["N"] - 2
    base = host_cert(libmpcg, r)
    sol = r["sol"].copy()
    sol[:, 3 * nx] += 1e-3
    cert = host_cert(libmpcg, r, sol)
    assert (np.abs(cert[:, 0] - 1e-3) <= base[:, 0] + tol(r)).all()
    np.testing.assert_array_equal(cert[:, 1:], base[:, 1:])
    for b in (0, len(sol) - 1):
        c, _ = numpy_kkt(oracle, r["P"], r["state"][b], r["coeffs"][b], sol[b])
        assert (np.abs(cert[b, :3] - c[:3]) <= tol(r)[b]).all()


def push_past_bound(r):
    """(rows, perturbed records): every row with a control on one of its bounds (published after
    honor_original_bounds: exactly on it), that control pushed 1e-3 beyond the bound."""
    N = r["N"]
    rows, sols = [], []
    for b in range(len(r["sol"])):
        xl, xu, _ = nlp_bounds(r["P"], r["state"][b])
        x = r["sol"][b, :8 * N - 2]
        at = np.flatnonzero(((x == xl) | (x == xu)) & (np.arange(8 * N - 2) >= 6 * N))
        if len(at):
            sol = r["sol"][b].copy()
            sol[at[0]] += 1e-3 if x[at[0]] == xu[at[0]] else -1e-3
            rows.append(b)
            sols.append(sol)
    return np.array(rows), np.array(sols)


@pytest.mark.parametrize("name", ["infinity", "bicycle_N25"])
def test_x_past_a_bound_raises_the_primal_column(libmpcg, oracle, tmp_path_factory, name):
    """A control that sits on its bound pushed 1e-3 beyond it: the bound violation, 1e-3, is the
    primal column (the defect rows the control enters move by d(turn)/d(w) 1e-3 or dt 1e-3, less).
    x also enters the gradient and the slacks, so columns 0 and 2 move too: every column is
    compared with numpy's evaluation of the same perturbed record."""
    r = records(name, oracle, tmp_path_factory)
    rows, sols = push_past_bound(r)
    assert len(rows) >= 16
    sub = dict(r, state=r["state"][rows], coeffs=r["coeffs"][rows])
    cert = host_cert(libmpcg, sub, sols)
    np.testing.assert_allclose(cert[:, 1], 1e-3, rtol=1e-9, atol=0)
    for i in range(0, len(rows), 8):
        c, s = numpy_kkt(oracle, r["P"], sub["state"][i], sub["coeffs"][i], sols[i])
        assert (np.abs(cert[i, :3] - c[:3]) <= 1e-11 * (1 + s)).all()


def test_invalid_parameter_row_gives_nan(libmpcg, oracle, tmp_path_factory):
    from mpc_ros_amd import params

    r = records("resto_N20", oracle, tmp_path_factory)
    rows = params.rows(r["P"], len(r["state"]))
    rows[1] = 0.0  # (DT = 0: outside mpcg_pparams_check's domains)
    cert = host_cert(libmpcg, r, rows=rows)
    assert np.isnan(cert[1]).all()
    keep = [0, 2, 3]
    np.testing.assert_array_equal(cert[keep], host_cert(libmpcg, r)[keep])


def test_stage_body_under_sanitizers(tmp_path):
    """tests/native/kkt_check.cpp: a stand-alone program over mpcg_kkt.h, built with ASan and UBSan
    and run directly."""
    exe = str(tmp_path / "kkt_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'mpc_ros_amd', 'csrc')}", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "kkt_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr
