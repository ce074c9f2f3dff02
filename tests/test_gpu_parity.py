"""GPU parity: the HIP kernel (through the C-ABI) against the oracle's fixtures and
the oracle itself, plus size-independent properties at the benchmark batch size.

Tolerance: the north star asks for (w, a) within 1e-6 of Ipopt; the kernel runs the
same algorithm as the oracle, so results are compared at 1e-7 (u0 and trajectory)
and must carry the same solver status.

Every row is compared, including those on which the oracle runs Ipopt's feasibility-
restoration phase (diag[:, 3] > 0): the device runs it too (k_resume_wide).
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, params_from_array

pytestmark = pytest.mark.gpu

ATOL = 1e-7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


def solver_for(P, **kw):
    from mpc_ros_amd.solver import BatchSolver

    return BatchSolver(0, P, **kw)


def check_against(r, g, min_same_iters=1.0):
    if "diag" in r:
        assert (r["diag"][:, 1] == 0).all()  # no filter entry dropped (Ipopt's filter is unbounded)
        if "diag" in g:  # the restoration phases, one for one
            np.testing.assert_array_equal(r["diag"][:, 0], g["diag"][:, 3])
    np.testing.assert_array_equal(r["status"], g["status"])
    np.testing.assert_allclose(r["u0"], g["u0"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(r["traj"], g["traj"], rtol=0, atol=ATOL)
    fin = np.isfinite(g["obj"])  # (the objective at a non-finite input is not compared)
    np.testing.assert_allclose(r["obj"][fin], g["obj"][fin], rtol=1e-9, atol=1e-7)
    assert np.mean(r["iters"] == g["iters"]) >= min_same_iters


def oracle_ref(oracle, P, st, cf, threads=16):
    return oracle.mpc_solve_batch(P, st, cf, opts=oracle.ref_opts(int(P["STEPS"])), nthreads=threads, diag=True)


def test_native_library_is_the_path(torch_cuda):
    from mpc_ros_amd import _lib

    L = _lib.lib()
    assert os.path.samefile(L._name, os.path.join(ROOT, "mpc_ros_amd", "libmpcg.so"))


def test_strategy_is_wave_and_lane_is_gone(torch_cuda):
    from mpc_ros_amd import params
    from mpc_ros_amd._lib import MpcgError

    assert solver_for(params.PLUGIN_DEFAULTS).strategy == "wave"
    with pytest.raises(MpcgError):
        solver_for(params.PLUGIN_DEFAULTS, strategy="lane")


def test_build_id_matches_sources(torch_cuda):
    """The loaded library was built from the sources in this tree (no stale binary)."""
    from mpc_ros_amd import _lib, build

    assert _lib.lib().mpcg_build_id().decode() == build.source_hash()


def test_infinity_set_matches_oracle(torch_cuda, infinity_golden):
    g = infinity_golden
    r = solver_for(params_from_array(g["params"])).solve(g["state"], g["coeffs"])
    check_against(r, g)


@pytest.mark.parametrize("name", ["class_defaults", "no_rate", "rate_w", "N40", "N3", "small_bound", "N80", "N100"])
def test_variants_match_oracle(torch_cuda, variants_golden, name):
    from test_core_host import SMALL_BOUND_ITERS_EXACT, SMALL_BOUND_ITERS_SLACK

    g = variants_golden[name]
    r = solver_for(params_from_array(g["params"])).solve(g["state"], g["coeffs"])
    # (small_bound: locally infeasible NLPs, every status and restoration count exact; see
    # test_core_host.SMALL_BOUND_ITERS_EXACT for the iteration counts allowed to differ)
    check_against(r, g, min_same_iters=SMALL_BOUND_ITERS_EXACT if name == "small_bound" else 1.0)
    if name == "small_bound":
        assert np.abs(r["iters"] - g["iters"]).max() <= SMALL_BOUND_ITERS_SLACK


@pytest.mark.parametrize("name", ["N20", "N40", "bicycle", "resto_N20", "resto_N40", "resto_N65"])
def test_ipopt_features_match_oracle(torch_cuda, features_golden, name):
    """Problems on which Ipopt's second-order corrections, watchdog, soft restoration and
    feasibility-restoration phase act (tests/golden/ipopt_features.npz; the resto_* sets:
    every problem of the scanned ranges that enters the restoration phase, run by the
    device's parked-problem kernel): same statuses and iteration counts."""
    g = features_golden[name]
    r = solver_for(g["P"]).solve(g["state"], g["coeffs"])
    check_against(r, g, min_same_iters=1.0)


def test_filter_beyond_lds_matches_oracle(torch_cuda, features_golden):
    """The filter holds filter_cap (64) entries in LDS and WideLayout::FX (448) more in the
    workspace, so no entry is dropped where Ipopt's unbounded filter keeps it: diag[:, 1]
    (entries dropped) is 0, diag[:, 3] reports the most entries held at once. The round-1
    advisor's problems 1887 and 16101 (N20 set) and resto_N40's problem 19304, whose
    filter reaches 196 entries (the workspace part in use), match the oracle; the peaks are
    those the host build of the same core reports (test_core_host.FILTER_PEAKS)."""
    from test_core_host import FILTER_PEAKS

    for name, peaks in FILTER_PEAKS.items():
        g = features_golden[name]
        r = solver_for(g["P"]).solve(g["state"], g["coeffs"])
        check_against(r, g, min_same_iters=1.0)
        assert (r["diag"][:, 1] == 0).all()
        for pid, peak in peaks.items():
            row = int(np.flatnonzero(g["index"] == pid)[0])
            assert r["diag"][row, 3] == peak


def test_cpu_time_budget_matches_oracle(torch_cuda, features_golden):
    """max_cpu_time forced low (0.005 s -> its iteration budget at N = 20): problems that
    need more iterations stop with status 14 (unknown, Ipopt's CPUTIME_EXCEEDED) at the
    budget, with the oracle's last iterate."""
    g = features_golden["budget"]
    r = solver_for(g["P"], max_cpu_time=float(g["max_cpu_time"])).solve(g["state"], g["coeffs"])
    check_against(r, g, min_same_iters=1.0)
    assert (r["status"] == 14).any() and (r["iters"] <= int(g["iter_budget"]) + 1).all()


def test_fresh_problems_against_oracle(torch_cuda, oracle):
    """Problems that are not in the fixtures, solved by both on this box."""
    from mpc_ros_amd import infinity, params

    idx = np.arange(900_000, 900_096)
    st, cf = infinity.make_problems(idx)
    P = params.PLUGIN_DEFAULTS
    ref = oracle_ref(oracle, P, st, cf)
    r = solver_for(P).solve(st, cf)
    check_against(r, ref)


def test_python_mpc_class_single_solves(torch_cuda, infinity_golden):
    from mpc_ros_amd.mpc import MPC

    g = infinity_golden
    m = MPC()
    m.LoadParams(params_from_array(g["params"]))
    for b in (0, 5, 100, 270):
        u = m.Solve(g["state"][b], g["coeffs"][b])
        np.testing.assert_allclose(u, g["u0"][b], atol=ATOL)
        np.testing.assert_allclose(m.mpc_x, g["traj"][b][0], atol=ATOL)
        np.testing.assert_allclose(m.mpc_theta, g["traj"][b][2], atol=ATOL)
        assert len(m.mpc_y) == 20 and m.last_status == g["status"][b]


def test_cpp_dropin_class(torch_cuda, tmp_path, infinity_golden):
    """The C++ drop-in MPC class, compiled the way the plugin would use it."""
    exe = str(tmp_path / "mpc_class")
    lib = os.path.join(ROOT, "mpc_ros_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "mpc_class_check.cpp"), "-L", lib, "-lmpcg",
                           "-L/opt/rocm/lib", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    g = infinity_golden
    lines = []
    for b in (0, 1, 2, 260):
        lines.append(" ".join(repr(float(v)) for v in np.concatenate([g["state"][b], g["coeffs"][b]])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         check=True).stdout.strip().split("\n")
    for line, b in zip(out, (0, 1, 2, 260)):
        vals = np.array(line.split(), dtype=float)
        np.testing.assert_allclose(vals[:2], g["u0"][b], atol=ATOL)
        np.testing.assert_allclose(vals[2:22], g["traj"][b][0], atol=ATOL)
        assert int(vals[-1]) == g["status"][b]


@pytest.mark.parametrize("B", [1, 63, 65, 200])
def test_ragged_batches(torch_cuda, infinity_golden, B):
    g = infinity_golden
    r = solver_for(params_from_array(g["params"])).solve(g["state"][:B], g["coeffs"][:B])
    np.testing.assert_allclose(r["u0"], g["u0"][:B], atol=ATOL)
    np.testing.assert_array_equal(r["status"], g["status"][:B])


def test_empty_batch(torch_cuda):
    from mpc_ros_amd import params

    r = solver_for(params.PLUGIN_DEFAULTS).solve(np.zeros((0, 6)), np.zeros((0, 4)))
    assert r["u0"].shape == (0, 2)


def test_full_size_properties(torch_cuda, oracle):
    """B = 65536 (the benchmark shard): every problem solves (status 1, the two that enter
    the restoration phase included); results are deterministic and independent of batch
    position; a random sample and every parked (restoration) problem agree with the
    oracle, restoration counts included; no filter entry is dropped."""
    torch = torch_cuda
    from mpc_ros_amd import infinity, params

    B = 65536
    P = params.PLUGIN_DEFAULTS
    st, cf = infinity.make_problems(np.arange(B))
    s = solver_for(P)
    dev = torch.device("cuda:0")
    tst, tcf = torch.from_numpy(st).to(dev), torch.from_numpy(cf).to(dev)
    outs = []
    for _ in range(2):
        u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
        traj = torch.empty((B, 3, 20), dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        diag = torch.empty((B, 4), dtype=torch.int32, device=dev)
        s.solve_device(tst, tcf, u0, traj, status, diag=diag)
        torch.cuda.synchronize()
        outs.append((u0.cpu().numpy(), traj.cpu().numpy(), status.cpu().numpy(), diag.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])  # deterministic
    np.testing.assert_array_equal(outs[0][3], outs[1][3])
    u0, traj, status, dg = outs[0]
    assert np.isfinite(u0).all() and np.isfinite(traj).all()
    assert (status == 1).all()
    assert (dg[:, 1] == 0).all()  # no filter entry dropped
    parked = np.flatnonzero(dg[:, 2] == 1)
    assert len(parked) >= 1 and (dg[parked, 0] >= 1).all() and (dg[dg[:, 2] == 0, 0] == 0).all()
    rng = np.random.default_rng(11)
    sample = np.union1d(np.sort(rng.choice(B, 48, replace=False)), parked)
    alone = s.solve(st[sample], cf[sample])
    np.testing.assert_array_equal(alone["u0"], u0[sample])  # batch-position invariance
    ref = oracle_ref(oracle, P, st[sample], cf[sample])
    np.testing.assert_array_equal(ref["status"], status[sample])
    np.testing.assert_array_equal(ref["diag"][:, 3], dg[sample, 0])
    np.testing.assert_allclose(u0[sample], ref["u0"], atol=ATOL)
    # controls inside the box (honor_original_bounds)
    assert np.abs(u0[:, 0]).max() <= P["ANGVEL"] and np.abs(u0[:, 1]).max() <= P["MAXTHR"]


def test_full_size_N40_restoration(torch_cuda, oracle):
    """B = 65536 at N = 40 (the 512-VGPR instance): every problem ends with status 1; every
    problem that went through the restoration phase (32) matches the oracle."""
    from mpc_ros_amd import infinity, params

    B = 65536
    P = dict(params.PLUGIN_DEFAULTS, STEPS=40)
    st, cf = infinity.make_problems(np.arange(B))
    r = solver_for(P).solve(st, cf)
    assert (r["status"] == 1).all() and (r["diag"][:, 1] == 0).all()
    parked = np.flatnonzero(r["diag"][:, 2] == 1)
    assert len(parked) >= 10
    ref = oracle_ref(oracle, P, st[parked], cf[parked])
    sub = {k: r[k][parked] for k in ("u0", "traj", "status", "obj", "iters", "diag")}
    check_against(sub, ref, min_same_iters=1.0)


def test_no_restoration_option_matches_oracle(torch_cuda, features_golden, oracle):
    """mpcg_params.no_restoration = 1 (the fp32 solver's setting) against the oracle with its
    restoration phase off: status 9 (or the acceptable point) where Ipopt would enter it,
    the same last iterate."""
    for name in ("resto_N20", "resto_N40"):
        g = features_golden[name]
        N = int(g["P"]["STEPS"])
        ref = oracle.mpc_solve_batch(g["P"], g["state"], g["coeffs"], opts=oracle.ref_opts(N, restoration=0),
                                     nthreads=8, diag=True)
        r = solver_for(g["P"], no_restoration=1).solve(g["state"], g["coeffs"])
        assert (r["diag"][:, 0] == 0).all() and (r["diag"][:, 2] == 0).all()
        assert (ref["status"] != 1).any()
        np.testing.assert_array_equal(r["status"], ref["status"])
        np.testing.assert_array_equal(r["iters"], ref["iters"])
        np.testing.assert_allclose(r["u0"], ref["u0"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(r["traj"], ref["traj"], rtol=0, atol=ATOL)
        # (a stopped iterate: resto_N40's 19304 stops after 99 iterations at an objective of
        # 2e8, where the two agree to 7e-8 relative)
        np.testing.assert_allclose(r["obj"], ref["obj"], rtol=1e-6)


def test_bicycle_matches_oracle(torch_cuda, bicycle_golden):
    """BASELINE configs[4]'s model (kinematic bicycle, N = 25) on the wavefront kernel."""
    g = bicycle_golden
    s = solver_for(g["P"])
    assert s.strategy == "wave"
    check_against(s.solve(g["state"], g["coeffs"]), g)


@pytest.mark.parametrize("N", [32, 33, 40, 80])
def test_bicycle_horizons_against_oracle(torch_cuda, oracle, N):
    """The bicycle model through each of its instance shapes -- the split sweeps (N = 32), the
    unsplit ones (33, and 40: the bicycle's long-horizon bench line) and two stage blocks (80) --
    against the oracle's bicycle restatement on problems outside the fixtures."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N, MODEL=1, LF=0.5, ANGVEL=0.5)
    st, cf = infinity.make_problems(np.arange(9700, 9708))
    check_against(solver_for(P).solve(st, cf), oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


@pytest.mark.parametrize("N", [65, 128])
def test_two_block_horizons(torch_cuda, oracle, N):
    """64 < STEPS <= 128: lane t carries stages t and 64 + t (the smallest and the largest
    two-block horizons), against the oracle."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9500, 9506))
    check_against(solver_for(P).solve(st, cf), oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


@pytest.mark.parametrize("N", [2, 32, 33])
def test_split_boundary_horizons(torch_cuda, oracle, N):
    """The smallest horizon the reference allows (STEPS = 2: one control stage) and both
    sides of the half-wave split's limit (32: split sweeps, 33: unsplit), against the
    oracle."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=N)
    st, cf = infinity.make_problems(np.arange(9600, 9612))
    check_against(solver_for(P).solve(st, cf), oracle_ref(oracle, P, st, cf), min_same_iters=1.0)


def test_steps_above_128_refused(torch_cuda):
    from mpc_ros_amd import infinity, params
    from mpc_ros_amd._lib import MpcgError

    st, cf = infinity.make_problems(np.arange(2))
    with pytest.raises(MpcgError):
        solver_for(dict(params.PLUGIN_DEFAULTS, STEPS=129)).solve(st, cf)


def test_full_width_N64(torch_cuda, oracle):
    """STEPS = 64: every lane of the wavefront carries a stage."""
    from mpc_ros_amd import infinity, params

    P = dict(params.PLUGIN_DEFAULTS, STEPS=64)
    sc = infinity.draw_scenarios(np.arange(300, 316))
    px, py, yaw, plan = infinity.scenario_poses(sc)
    st, cf = infinity.find_best_path(px, py, yaw, sc["v"], sc["w_prev"], sc["a_prev"], P["DT"], plan, True)
    g = oracle_ref(oracle, P, st, cf)
    check_against(solver_for(P).solve(st, cf), g, min_same_iters=1.0)


def test_nonfinite_inputs(torch_cuda, oracle):
    """NaN / inf inputs end before the first iteration with INVALID_NUMBER_DETECTED
    (11), as in the oracle; the other problems of the batch are unaffected."""
    from mpc_ros_amd import params
    from test_core_host import nonfinite_inputs

    P = params.PLUGIN_DEFAULTS
    st, cf = nonfinite_inputs()
    g = oracle_ref(oracle, P, st, cf, threads=4)
    r = solver_for(P).solve(st, cf)
    check_against(r, g, min_same_iters=1.0)
    assert (g["status"] == 11).sum() == 5  # (row 2, a huge finite state: in the restoration phase)


def test_solve_multi_one_gpu_matches_single(torch_cuda, infinity_golden):
    """mpcg_solve_multi (one process, RCCL gather to devices[0]) on the GPUs of this box:
    results equal the single-handle solve bitwise."""
    import torch

    from mpc_ros_amd.solver import solve_multi

    g = infinity_golden
    P = params_from_array(g["params"])
    devs = list(range(torch.cuda.device_count()))
    r = solve_multi(devs, P, g["state"], g["coeffs"])
    s = solver_for(P).solve(g["state"], g["coeffs"])
    for k in ("u0", "traj", "status", "iters", "obj"):
        np.testing.assert_array_equal(r[k], s[k])


def test_multi_context_matches_single(torch_cuda, infinity_golden):
    """The persistent multi-GPU context (mpcg_multi: communicator, handles and buffers created
    once) on the GPUs of this box: several batches of different sizes through one context
    equal the single-handle solve bitwise; a batch above its B_max is refused."""
    import torch

    from mpc_ros_amd._lib import MpcgError
    from mpc_ros_amd.solver import MultiSolver

    g = infinity_golden
    P = params_from_array(g["params"])
    devs = list(range(torch.cuda.device_count()))
    m = MultiSolver(devs, 288, P)
    s = solver_for(P)
    for B in (288, 5, 131):
        r = m.solve(g["state"][:B], g["coeffs"][:B])
        ref = s.solve(g["state"][:B], g["coeffs"][:B])
        for k in ("u0", "traj", "status", "iters", "obj"):
            np.testing.assert_array_equal(r[k], ref[k])
    with pytest.raises(MpcgError):
        m.solve(np.zeros((289, 6)), np.zeros((289, 4)))
    m.close()


def test_default_option_instance_equals_general(torch_cuda, features_golden, oracle):
    """The kernel instance that compiles the reference's (default) Ipopt options as
    constants and the general instance (taken for any other option values) run the same
    solver: an option change that cannot act (acceptable_obj_change_tol 1e20 -> 1e30)
    takes the general instance and must give bitwise the same results; an option that acts
    (no second-order corrections, no watchdog) must match the oracle under that option."""
    g = features_golden["N20"]
    a = solver_for(g["P"]).solve(g["state"], g["coeffs"])
    b = solver_for(g["P"], acceptable_obj_change_tol=1e30).solve(g["state"], g["coeffs"])
    for k in ("u0", "traj", "status", "iters", "obj"):
        np.testing.assert_array_equal(a[k], b[k])
    c = solver_for(g["P"], max_soc=0, watchdog_shortened_iter_trigger=0).solve(g["state"], g["coeffs"])
    o = oracle.ref_opts(20)
    o.max_soc = 0
    o.watchdog_shortened_iter_trigger = 0
    ref = oracle.mpc_solve_batch(g["P"], g["state"], g["coeffs"], opts=o, nthreads=8, diag=True)
    check_against(c, ref, min_same_iters=1.0)


@pytest.mark.parametrize("name", ["N40", "N64", "bicycle", "bicycle_N40"])
def test_default_option_instances_equal_general(torch_cuda, features_golden, variants_golden, bicycle_golden,
                                                oracle, name):
    """Every other fp64 configuration's default-options instance (N = 33..64 at two
    wavefronts per SIMD, N = 64's one-wavefront instance, configs[4]'s bicycle, the bicycle
    at N = 40) against the general instance bitwise -- fixture rows (restoration, SOC and
    watchdog rows included) and the oracle on the same rows."""
    from mpc_ros_amd import infinity, params

    if name == "N40":
        g = variants_golden["N40"]
        P, st, cf = params_from_array(g["params"]), g["state"], g["coeffs"]
        f = features_golden["resto_N40"]
        st, cf = np.concatenate([st, f["state"]]), np.concatenate([cf, f["coeffs"]])
    elif name == "bicycle":
        g, f = bicycle_golden, features_golden["bicycle"]
        P, st, cf = g["P"], np.concatenate([g["state"], f["state"]]), np.concatenate([g["coeffs"], f["coeffs"]])
    else:
        P = dict(params.PLUGIN_DEFAULTS, STEPS=64 if name == "N64" else 40)
        if name == "bicycle_N40":
            P.update(MODEL=1, LF=0.5, ANGVEL=0.5)
        st, cf = infinity.make_problems(np.arange(7000, 7032))
    sa, sb = solver_for(P), solver_for(P, acceptable_obj_change_tol=1e30)
    a, b = sa.solve(st, cf), sb.solve(st, cf)
    # (k_solve_wide<model,split,type,blocks,default options,waves per SIMD>: only the fifth differs)
    ka, kb = sa.last_kernel[:-1].split(","), sb.last_kernel[:-1].split(",")
    assert ka[4] == "true" and kb[4] == "false" and ka[:4] + ka[5:] == kb[:4] + kb[5:], (ka, kb)
    for k in ("u0", "traj", "status", "iters", "obj"):
        np.testing.assert_array_equal(a[k], b[k])
    ref = oracle.mpc_solve_batch(P, st, cf, opts=oracle.ref_opts(int(P["STEPS"])), nthreads=16, diag=True)
    check_against(a, ref)
