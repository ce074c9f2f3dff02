"""GPU parity of the Riccati sweep with the affine part as a ninth column of its lane grid
(wide_core.h riccati9(): from the M-column reads to the store of the cost-to-go, lane t < 63 owns
entry (t / 9, t % 9) of [P | p], rows 0..6; a column-8 lane runs a P column's instruction stream
on p's operands, a row-6 lane gives row 7's entry, p and the coupling constants live in the M
scratch's padding).

Fresh infinity problems at the horizons where the sweep's cases differ -- N = 2 (the terminal
stage plus one step), 3, the benchmark's 20, 33 (unsplit sweeps, the gain records in the
workspace) and 65 (two stage blocks) -- the bicycle at N = 25 (its heading-rate terms and the
(v, w) curvature addend), and one batch through the benchmark's own instance (B = 4,097) whose
first rows are the fixture rows of the paths that repeat Newton solves at one iterate
(second-order corrections, inertia correction) or leave the sweep for the restoration problem's
and come back (soft restoration, restoration).  Compared as tests/test_gpu_parity.py does: status
and iteration count exact, u0 and trajectory within 1e-7 of the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import params_from_array
from test_fused_sweeps_host import INERTIA_ROW, SOC_ROW
from test_gpu_headline import HEADLINE
from test_gpu_parity import check_against, oracle_ref, solver_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


@pytest.mark.parametrize("N,B", [(2, 64), (3, 64), (20, 64), (33, 64), (65, 8)])
def test_fresh_problems(torch_cuda, oracle, N, B):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9900, 9900 + B))
    r = solver_for(P).solve(st, cf)
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_fresh_problems_bicycle(torch_cuda, oracle):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=25, MODEL=1, LF=0.5, ANGVEL=0.5)
    st, cf = infinity.make_problems(np.arange(9900, 9964))
    r = solver_for(P).solve(st, cf)
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def _rows(g, rows):
    return {k: g[k][rows] for k in ("state", "coeffs", "u0", "traj", "status", "iters", "obj", "diag")}


def _first(g, col):
    """The first row of a fixture set whose diag column col is positive."""
    return int(np.flatnonzero(g["diag"][:, col] >= 1)[0])


def test_headline_instance_with_the_rare_path_rows(torch_cuda, oracle, infinity_golden, features_golden):
    """B = 4,097: the smallest batch the benchmark's instance takes.  Its first rows: the
    inertia-correction and second-order-correction rows of the infinity set, a second-order,
    a soft-restoration and a restoration row of the feature set, a row of the restoration set."""
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    f, fr = features_golden["N20"], features_golden["resto_N20"]
    assert params_from_array(infinity_golden["params"]) == P and f["P"] == P and fr["P"] == P
    parts = [_rows(infinity_golden, [INERTIA_ROW, SOC_ROW]), _rows(f, [_first(f, 0), _first(f, 2), _first(f, 3)]),
             _rows(fr, [0])]
    g = {k: np.concatenate([x[k] for x in parts]) for k in parts[0]}
    assert g["diag"][1, 0] >= 1 and g["diag"][3, 2] >= 1 and g["diag"][4, 3] >= 1 and g["diag"][5, 3] >= 1
    n = len(g["state"])
    st, cf = infinity.make_problems(np.arange(31_000, 31_000 + 4097 - n))
    s = solver_for(P)
    r = s.solve(np.concatenate([g["state"], st]), np.concatenate([g["coeffs"], cf]))
    assert s.last_kernel == HEADLINE
    keys = ("u0", "traj", "status", "iters", "obj", "diag")
    check_against({k: r[k][:n] for k in keys}, g, min_same_iters=1.0)
    check_against({k: r[k][n:] for k in keys}, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)
