"""GPU parity of the split solver's fused sweeps (wide_core.h: the statistics sweep writes the
Newton system's stage data and takes an accepted trial point's sums from the trial sweep).

Fresh infinity problems at the horizons where the split sweeps' cases first differ (N = 2, 3,
4: k == 0, last, k <= N - 3; 32: full half-waves) and at the benchmark's N = 20, on the
fixture-sized instance (B = 64) and on the two-wavefronts-per-SIMD instance (B = 4,097); the
bicycle at N = 25; and one row for each rare path that invalidates or bypasses the stage
table's validity record: an inertia-correction row, a second-order-correction row, a watchdog
row and a restoration row (the resume kernel's unpark).  Compared as tests/test_gpu_parity.py
does: status and iteration count exact, u0 and trajectory within 1e-7 of the oracle.
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
def test_fresh_problems_at_split_horizons(torch_cuda, oracle, N):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9900, 9964))
    s = solver_for(P)
    r = s.solve(st, cf)
    assert s.last_kernel == LONE
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_fresh_problems_two_per_simd_instance(torch_cuda, oracle):
    """B = 4,097: the smallest batch the benchmark's instance takes."""
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    st, cf = infinity.make_problems(np.arange(20_000, 20_000 + 4097))
    s = solver_for(P)
    r = s.solve(st, cf)
    assert s.last_kernel == HEADLINE
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_fresh_problems_bicycle(torch_cuda, oracle):
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=25, MODEL=1, LF=0.5, ANGVEL=0.5)
    st, cf = infinity.make_problems(np.arange(9900, 9964))
    s = solver_for(P)
    r = s.solve(st, cf)
    assert s.last_kernel == "k_solve_wide<1,true,double,1,true,2>"  # (the bicycle's one default-option split instance)
    check_against(r, oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def _rows(g, rows):
    return {k: g[k][rows] for k in ("state", "coeffs", "u0", "traj", "status", "iters", "obj", "diag")}


@pytest.mark.parametrize("path", ["inertia", "soc", "watchdog", "restoration"])
def test_rare_paths_through_the_fused_sweeps(torch_cuda, infinity_golden, features_golden, path):
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
        g, P = _rows(f, [int(np.flatnonzero(f["diag"][:, 1] >= 1)[0])]), f["P"]
    else:
        f = features_golden["resto_N20"]
        g, P = _rows(f, [0]), f["P"]
        assert g["diag"][0, 3] >= 1
    s = solver_for(P)
    r = s.solve(g["state"], g["coeffs"])
    assert s.last_kernel.startswith("k_solve_wide<%d,true,double,1," % int(P.get("MODEL", 0)))
    check_against(r, g, min_same_iters=1.0)
