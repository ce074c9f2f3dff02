"""The split solver's kept reciprocal slacks against the build without them, on the host (no
GPU needed).

tests/native/wide_slack_check.cpp is built twice from mpc_ros_amd/csrc/wide_core.h: as the
product compiles it (MPCG_FUSE bits 2 and 3: the split accept pass and the statistics sweep keep
rcp(w - lo), rcp(hi - w) of their lane's four variables, and the statistics, the step statistics
and the next accept pass at the same iterate take them), and with
-DMPCG_FUSE=3 (every sweep forms its own).  A kept reciprocal is the same function of the same
bits, so the two programs must print the same bytes: status, iteration count,
inertia-correction retries and the final iterate (w, z_L, z_U, the step, y) of every problem,
bit for bit -- double and float (the float solver keeps none under either setting: wide_core.h
FUSE_RC follows FUSE_SQ).
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from conftest import params_from_array
from host_harness import build_all, harness_stdin, opts_line
from test_core_host import fp32_opts
from test_fused_sweeps_host import SETS, fixture_sets



@pytest.fixture(scope="module")
def programs():
    """{(dtype, kept)}: the four builds of the harness."""
    keys = [(ty, kept) for ty in ("double", "float") for kept in (True, False)]
    flags = [(f"-DHOST_T={ty}",) + (() if kept else ("-DMPCG_FUSE=3",)) for ty, kept in keys]
    return dict(zip(keys, build_all("wide_slack_check", flags)))


def run(exe, P, state, coeffs, o):
    out = subprocess.run([exe], input=harness_stdin(P, state, coeffs, o, opts_line(o)), capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(state) + 1
    words = out[-1].split()  # "sweeps <all> cached <n>"
    return out[:-1], int(words[1]), int(words[3])


def both(programs, ty, P, state, coeffs, oracle):
    """The two builds on the same problems: equal output; the default build's rows and its
    (consumer sweeps, sweeps that took the kept reciprocals) counts."""
    N = int(P["STEPS"])
    o = oracle.ref_opts(N) if ty == "double" else fp32_opts(oracle, N)
    kept, n_all, n_cached = run(programs[ty, True], P, state, coeffs, o)
    formed, n_all0, n_cached0 = run(programs[ty, False], P, state, coeffs, o)
    assert n_cached0 == 0 and n_all0 == n_all  # (the MPCG_FUSE=3 build forms them in every sweep)
    bad = [b for b in range(len(state)) if kept[b] != formed[b]]
    assert not bad, (ty, bad[:8], [kept[b].split()[:3] + formed[b].split()[:3] for b in bad[:4]])
    return kept, n_all, n_cached


@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("name", SETS)
def test_kept_equals_formed_on_fixtures(programs, oracle, infinity_golden, features_golden, variants_golden,
                                        bicycle_golden, name, ty):
    P, g = fixture_sets(infinity_golden, features_golden, variants_golden, bicycle_golden)[name]
    rows, n_all, n_cached = both(programs, ty, P, g["state"], g["coeffs"], oracle)
    if name == "infinity":
        # the share of consumer sweeps (statistics sweeps and step-statistics sweeps) that took the
        # kept reciprocals (DESIGN.md quotes the double build's figure): both branches ran -- a
        # statistics sweep without an accept pass before it (the first of a solve, the one after
        # the watchdog's or the restoration phase's return) forms its own
        print(f"infinity fixture rows, {ty}: {n_cached} of {n_all} consumer sweeps took the kept "
              f"reciprocal slacks ({n_cached / n_all:.3f}), {n_all - n_cached} formed them")
        if ty == "float":
            assert n_cached == 0  # (the fp32 solver keeps none: wide_core.h FUSE_RC)
        else:
            assert n_cached > 0 and n_all - n_cached > 0
            np.testing.assert_array_equal([int(r.split()[0]) for r in rows], g["status"])
            np.testing.assert_array_equal([int(r.split()[1]) for r in rows], g["iters"])


@pytest.mark.parametrize("ty", ["double", "float"])
@pytest.mark.parametrize("N", [2, 3, 4, 32])
def test_kept_equals_formed_at_boundary_horizons(programs, oracle, N, ty):
    """Fresh infinity problems at the horizons where the sweeps' k == 0, last and
    full-half-wave cases first differ."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9800, 9812))
    both(programs, ty, P, st, cf, oracle)
