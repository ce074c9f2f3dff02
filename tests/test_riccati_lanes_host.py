"""The Riccati sweep with the affine part as a ninth column of its lane grid against the sweep in
which every lane of a row forms p_i, on the host (no GPU needed).

tests/native/wide_ric_check.cpp is built twice from mpc_ros_amd/csrc/wide_core.h: as the product
compiles it (MPCG_RIC9: from the M-column reads to the store of the cost-to-go, lane t < 63 owns
entry (t / 9, t % 9) of [P | p], rows 0..6, a column-8 lane running a P column's instruction
stream on p's operands, and a row-6 lane giving row 7's entry), and with -DMPCG_RIC9=0
(riccati()'s own body).  The new sweep evaluates the same expressions on the same bits, so the
two programs must print the same bytes: status, iteration count, inertia-correction retries, the
final iterate (w, z_L, z_U, the step, y) and a running hash of every sweep's gain records (the
18 values per stage as the step recursion reads them), bit for bit -- double and float (the
float solver keeps riccati()'s body under either setting: on the device its outputs moved with
the new sweep, wide_core.h RIC9).  The restoration problem keeps riccati()'s body as well; the
solver that continues after it takes the new sweep.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from host_harness import build_all, harness_stdin, opts_line
from test_core_host import fp32_opts
from test_fused_sweeps_host import INERTIA_ROW, SETS, SOC_ROW, fixture_sets


@pytest.fixture(scope="module")
def programs():
    """{(dtype, ninth)}: the four builds of the harness."""
    keys = [(ty, ninth) for ty in ("double", "float") for ninth in (True, False)]
    flags = [(f"-DHOST_T={ty}",) + (() if ninth else ("-DMPCG_RIC9=0",)) for ty, ninth in keys]
    return dict(zip(keys, build_all("wide_ric_check", flags)))


def run(exe, P, state, coeffs, o):
    out = subprocess.run([exe], input=harness_stdin(P, state, coeffs, o, opts_line(o)), capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(state) + 1
    return out[:-1], int(out[-1].split()[1])  # "sweeps <n>"


def both(programs, ty, P, state, coeffs, oracle):
    """The two builds on the same problems: equal output; the default build's rows and its
    count of sweeps."""
    N = int(P["STEPS"])
    o = oracle.ref_opts(N) if ty == "double" else fp32_opts(oracle, N)
    new, n_new = run(programs[ty, True], P, state, coeffs, o)
    old, n_old = run(programs[ty, False], P, state, coeffs, o)
    bad = [b for b in range(len(state)) if new[b] != old[b]]
    assert not bad, (ty, bad[:8], [new[b].split()[:4] + old[b].split()[:4] for b in bad[:4]])
    assert n_new == n_old and n_new >= len(state)
    return new, n_new


@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("name", SETS)
def test_ninth_column_equals_row_lanes_on_fixtures(programs, oracle, infinity_golden, features_golden,
                                                   variants_golden, bicycle_golden, name, ty):
    P, g = fixture_sets(infinity_golden, features_golden, variants_golden, bicycle_golden)[name]
    rows, n = both(programs, ty, P, g["state"], g["coeffs"], oracle)
    print(f"{name}, {ty}: {n} sweeps over {len(rows)} problems")
    if ty == "double" and name == "infinity":
        np.testing.assert_array_equal([int(r.split()[0]) for r in rows], g["status"])
        np.testing.assert_array_equal([int(r.split()[1]) for r in rows], g["iters"])
        # the rows with repeated solves at one iterate take them
        assert int(rows[INERTIA_ROW].split()[2]) >= 1 and g["diag"][SOC_ROW, 0] >= 1
    if ty == "double" and name == "features_resto_N20":
        assert (g["diag"][:, 3] >= 1).any()  # (restoration phases: riccati()'s body, then the new sweep again)


# N = 2: the terminal stage plus one step; 3, 4: k == 0 and the last step apart; 32: full
# half-waves; 33: unsplit, the gain records in the workspace; 65: two stage blocks
@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("N", [2, 3, 4, 32, 33, 65])
def test_ninth_column_equals_row_lanes_at_boundary_horizons(programs, oracle, N, ty):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9800, 9812))
    both(programs, ty, P, st, cf, oracle)
