"""The split solver's fused sweeps against its separate passes, on the host (no GPU needed).

tests/native/wide_fused_check.cpp is built twice from mpc_ros_amd/csrc/wide_core.h: as the
product compiles it (the statistics sweep writes the Newton system's stage data, and takes an
accepted trial point's objective, log-barrier and violation sums from the trial sweep), and
with -DMPCG_FUSE=0 (the stage-data pass before every Riccati sweep, every sum evaluated and
reduced again).  Fusing changes no operand and no operation, so the two programs must print
the same bytes: status, iteration count, inertia-correction retries and the final iterate
(w, z_L, z_U, the step, y) of every problem, bit for bit -- double and float (the float solver
keeps its separate passes under either setting: its fused sweeps moved the device's fp32
outputs, wide_core.h FUSE_SQ).
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from conftest import params_from_array
from host_harness import build_all, harness_stdin, opts_line
from test_core_host import fp32_opts

# rows of the infinity fixture set the GPU test (tests/test_gpu_fused_sweeps.py) runs for their
# rare paths: INERTIA_ROW repeats Newton solves with a Hessian perturbation (and takes no
# second-order correction), SOC_ROW accepts second-order corrections
INERTIA_ROW, SOC_ROW = 9, 7


@pytest.fixture(scope="module")
def programs():
    """{(dtype, fused)}: the four builds of the harness."""
    keys = [(ty, fused) for ty in ("double", "float") for fused in (True, False)]
    flags = [(f"-DHOST_T={ty}",) + (() if fused else ("-DMPCG_FUSE=0",)) for ty, fused in keys]
    return dict(zip(keys, build_all("wide_fused_check", flags)))


def run(exe, P, state, coeffs, o):
    out = subprocess.run([exe], input=harness_stdin(P, state, coeffs, o, opts_line(o)), capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(state) + 1
    words = out[-1].split()  # "solves <all> skipped <n>"
    return out[:-1], int(words[1]), int(words[3])


def both(programs, ty, P, state, coeffs, oracle):
    """The fused and the separate build on the same problems: equal output; the fused build's
    rows and its (solves, skipped) counts."""
    N = int(P["STEPS"])
    o = oracle.ref_opts(N) if ty == "double" else fp32_opts(oracle, N)
    fused, n_all, n_skip = run(programs[ty, True], P, state, coeffs, o)
    sep, n_all0, n_skip0 = run(programs[ty, False], P, state, coeffs, o)
    assert n_skip0 == 0 and n_all0 == n_all  # (the separate build runs the stage-data pass every time)
    bad = [b for b in range(len(state)) if fused[b] != sep[b]]
    assert not bad, (ty, bad[:8], [fused[b].split()[:3] + sep[b].split()[:3] for b in bad[:4]])
    return fused, n_all, n_skip


def fixture_sets(infinity_golden, features_golden, variants_golden, bicycle_golden):
    """Every fixture set the split solver takes at N = 20, and the bicycle set (N = 25)."""
    sets = {"infinity": (params_from_array(infinity_golden["params"]), infinity_golden)}
    for name in ("N20", "resto_N20"):
        sets["features_" + name] = (features_golden[name]["P"], features_golden[name])
    for name in ("class_defaults", "rate_w", "no_rate", "small_bound"):
        sets["variants_" + name] = (params_from_array(variants_golden[name]["params"]), variants_golden[name])
    for P, _ in sets.values():
        assert P["STEPS"] == 20
    sets["bicycle"] = (bicycle_golden["P"], bicycle_golden)
    assert bicycle_golden["P"]["STEPS"] == 25
    return sets


SETS = ["infinity", "features_N20", "features_resto_N20", "variants_class_defaults", "variants_rate_w",
        "variants_no_rate", "variants_small_bound", "bicycle"]


@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("name", SETS)
def test_fused_equals_separate_on_fixtures(programs, oracle, infinity_golden, features_golden, variants_golden,
                                           bicycle_golden, name, ty):
    P, g = fixture_sets(infinity_golden, features_golden, variants_golden, bicycle_golden)[name]
    rows, n_all, n_skip = both(programs, ty, P, g["state"], g["coeffs"], oracle)
    if name == "infinity":
        # the share of Newton solves that skipped the stage-data pass (DESIGN.md quotes the double
        # build's figure): both branches ran
        print(f"infinity fixture rows, {ty}: {n_skip} of {n_all} Newton solves skipped the stage-data pass "
              f"({n_skip / n_all:.3f})")
        if ty == "float":
            assert n_skip == 0  # (the fp32 solver keeps its separate passes: wide_core.h FUSE_SQ)
        else:
            assert 0 < n_skip / n_all < 1
            np.testing.assert_array_equal([int(r.split()[0]) for r in rows], g["status"])
            np.testing.assert_array_equal([int(r.split()[1]) for r in rows], g["iters"])
            # the rows the GPU test names for their rare paths take them
            assert int(rows[INERTIA_ROW].split()[2]) >= 1 and g["diag"][INERTIA_ROW, 0] == 0
            assert g["diag"][SOC_ROW, 0] >= 1


@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("N", [2, 3, 4, 32])
def test_fused_equals_separate_at_boundary_horizons(programs, oracle, N, ty):
    """Fresh infinity problems at the horizons where the sweeps' k == 0, last, k <= N - 3 and
    full-half-wave cases first differ."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9800, 9812))
    both(programs, ty, P, st, cf, oracle)
