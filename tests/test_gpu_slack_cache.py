"""GPU parity of the split solver's kept reciprocal slacks (wide_core.h FUSE_RC, FUSE_AC: the
split accept pass and the statistics sweep keep rcp(w - lo), rcp(hi - w) of their lane's four
variables in registers, and the statistics, the step statistics and the next accept pass at the
same iterate take them instead of forming them again; the benchmark's instance keeps them, the
others run the same sweeps without).

Fresh infinity problems at the horizons where the split sweeps' cases first differ (N = 2, 3,
4: k == 0, last; 32: full half-waves) and at the benchmark's N = 20, on the fixture-sized
instance (B = 64) and on the two-wavefronts-per-SIMD instance (B = 4,097); the bicycle at
N = 25; and one fixture row for each path that replaces the iterate in LDS and so clears the
record of what the registers hold: a watchdog row, a soft-restoration row, a restoration row
(the resume kernel's unpark), and, for the solves that repeat at one iterate, a
second-order-correction row and an inertia-correction row.  Compared as
tests/test_gpu_parity.py does: status and iteration count exact, u0 and trajectory within 1e-7
of the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import params_from_array
from test_fused_sweeps_host import INERTIA_ROW, SOC_ROW
from test_gpu_headline import HEADLINE, LONE
from test_gpu_parity import check_against, oracle_ref, solver_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


@pytest.mark.parametrize("N", [2, 3, 4, 20, 32])
def test_fresh_problems_through_the_lone_instance(torch_cuda, oracle, N):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9700, 9764))
    s = solver_for(P)
    r = s.solve(st, cf)
    assert s.last_kernel == LONE
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_fresh_problems_through_the_headline_instance(torch_cuda, oracle, infinity_golden, features_golden):
    """B = 4,097: the smallest batch the benchmark's instance takes -- the one instance that
    keeps the reciprocals.  Its first rows are the N = 20 fixture rows of the paths that clear
    the record there (soft restoration, restoration and unpark) or repeat solves at one iterate
    (second-order corrections, inertia correction)."""
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    f, fr = features_golden["N20"], features_golden["resto_N20"]
    assert params_from_array(infinity_golden["params"]) == P and f["P"] == P and fr["P"] == P
    parts = [_rows(infinity_golden, [INERTIA_ROW, SOC_ROW]), _rows(f, [_first(f, 0), _first(f, 2), _first(f, 3)]),
             _rows(fr, [0])]
    g = {k: np.concatenate([x[k] for x in parts]) for k in parts[0]}
    assert g["diag"][1, 0] >= 1 and g["diag"][3, 2] >= 1 and g["diag"][4, 3] >= 1 and g["diag"][5, 3] >= 1
    n = len(g["state"])
    st, cf = infinity.make_problems(np.arange(30_000, 30_000 + 4097 - n))
    s = solver_for(P)
    r = s.solve(np.concatenate([g["state"], st]), np.concatenate([g["coeffs"], cf]))
    assert s.last_kernel == HEADLINE
    keys = ("u0", "traj", "status", "iters", "obj", "diag")
    check_against({k: r[k][:n] for k in keys}, g, min_same_iters=1.0)
    check_against({k: r[k][n:] for k in keys}, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_fresh_problems_bicycle(torch_cuda, oracle):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=25, MODEL=1, LF=0.5, ANGVEL=0.5)
    st, cf = infinity.make_problems(np.arange(9700, 9764))
    s = solver_for(P)
    r = s.solve(st, cf)
    assert s.last_kernel == "k_solve_wide<1,true,double,1,true,2>"  # (the bicycle's one default-option split instance)
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def _rows(g, rows):
    return {k: g[k][rows] for k in ("state", "coeffs", "u0", "traj", "status", "iters", "obj", "diag")}


def _first(g, col):
    """The first row of a fixture set whose diag column col is positive."""
    return int(np.flatnonzero(g["diag"][:, col] >= 1)[0])


@pytest.mark.parametrize("path", ["watchdog", "soft", "restoration", "soc", "inertia"])
def test_paths_that_clear_or_outlive_the_record(torch_cuda, infinity_golden, features_golden, path):
    """diag columns of the fixtures: second-order corrections, watchdog activations, soft
    restoration steps, restoration phases.  (The inertia-correction row is named by the host
    emulation, which counts its repeated Newton solves: tests/test_fused_sweeps_host.py.)"""
    if path == "inertia":
        g, P = _rows(infinity_golden, [INERTIA_ROW]), params_from_array(infinity_golden["params"])
    elif path == "soc":
        g, P = _rows(infinity_golden, [SOC_ROW]), params_from_array(infinity_golden["params"])
        assert g["diag"][0, 0] >= 1
    elif path == "watchdog":
        f = features_golden["bicycle"]
        g, P = _rows(f, [_first(f, 1)]), f["P"]
        assert g["diag"][0, 1] >= 1
    elif path == "soft":
        f = features_golden["N20"]
        g, P = _rows(f, [_first(f, 2)]), f["P"]
        assert g["diag"][0, 2] >= 1
    else:
        f = features_golden["resto_N20"]
        g, P = _rows(f, [0]), f["P"]
        assert g["diag"][0, 3] >= 1
    s = solver_for(P)
    r = s.solve(g["state"], g["coeffs"])
    assert s.last_kernel.startswith("k_solve_wide<%d,true,double,1," % int(P.get("MODEL", 0)))
    check_against(r, g, min_same_iters=1.0)
