"""GPU: the sensitivity kernel k_sens (mpcg_sens_device) and the correction k_sens_apply on the
records the GPU solver wrote, against the host entry mpcg_sens and the dense numpy solve of
tests/test_sens_host.py.

Kernel and host entry run the same phases in the same order without FMA contraction; they differ by
the platform's sin / cos (a few ulp) in the stage data.  SENS_DEVICE_MEASURED is the largest
max |delta| / max(1, max |G|) of gain and dx between them over the shapes below
(test_kernel_equals_the_host_entry prints every shape's figure); the bound is ten times it, capped
at 1e-9.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import solver_for, torch_cuda  # noqa: F401
from test_gpu_solution import dev
from test_sens_host import (SENS_DENSE_BOUND, apply_case, apply_rule, dense_reference, flag_records, records, rel_err)
from test_solution_host import fixture_set

pytestmark = pytest.mark.gpu

SENS_DEVICE_MEASURED = 6.861e-14  # variants_N80; 7.1e-15 at the headline horizon
SENS_DEVICE_BOUND = min(10 * SENS_DEVICE_MEASURED, 1e-9)

# the smallest shapes that reach every path: one control without a rate neighbour (N = 3), the
# headline horizon, the bicycle, an unsplit horizon, the lane loop past stage 63 (N = 65, 80), one
# problem, and more problems than one CU holds
SHAPES = {"variants_N3": None, "infinity": slice(0, 24), "bicycle_N25": slice(0, 6), "variants_N40": slice(0, 3),
          "resto_N65": None, "variants_N80": None, "B1": slice(1, 2), "B130": None,
          # problems away from the infinity course (tests/golden/general.npz)
          "general_N20": None, "general_bicycle_N25": None}
_solved = {}


def shape_batch(name):
    if name in ("B1", "B130"):
        P, g = fixture_set("infinity")
        idx = np.arange(130) % 24 if name == "B130" else np.arange(1, 2)
        return P, np.ascontiguousarray(g["state"][idx]), np.ascontiguousarray(g["coeffs"][idx])
    P, g = fixture_set(name)
    sel = SHAPES[name] or slice(None)
    return P, np.ascontiguousarray(g["state"][sel]), np.ascontiguousarray(g["coeffs"][sel])


def solve_and_sens(torch, s, st, cf, sol_in=None, rows=None, want_dx=True):
    """mpcg_solve_device_sol then mpcg_sens_device on the same stream (sol_in: the sensitivities of
    these records instead, no solve); the outputs as numpy arrays."""
    from mpc_ros_amd.solver import solution_elems

    B, N = len(st), s.N
    d = torch.device("cuda:0")
    tst, tcf = dev(torch, st), dev(torch, cf)
    u0 = torch.full((B, 2), 7.0, dtype=torch.float64, device=d)
    status = torch.full((B,), -1, dtype=torch.int32, device=d)
    sol = torch.full((B, solution_elems(N)), 7.0, dtype=torch.float64, device=d) if sol_in is None else dev(torch, sol_in)
    gain = torch.full((B, 2, 10), 7.0, dtype=torch.float64, device=d)
    dx = torch.full((B, 10, 8 * N - 2), 7.0, dtype=torch.float64, device=d) if want_dx else None
    info = torch.full((B,), -1, dtype=torch.int32, device=d)
    if sol_in is None:
        s.solve_device(tst, tcf, u0, status=status, sol=sol)
    s.sens_device(tst, tcf, sol, gain, dx=dx, info=info, pparams=None if rows is None else dev(torch, rows))
    torch.cuda.synchronize()
    out = dict(u0=u0, status=status, sol=sol, gain=gain, info=info)
    if want_dx:
        out["dx"] = dx
    return {k: v.cpu().numpy() for k, v in out.items()}


def solved(torch, name):
    """A shape's solve and sensitivities on the GPU, once; never modified."""
    if name not in _solved:
        P, st, cf = shape_batch(name)
        s = solver_for(P)
        r = solve_and_sens(torch, s, st, cf)
        r.update(P=P, N=int(P["STEPS"]), state=st, coeffs=cf, solver=s)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _solved[name] = r
    return _solved[name]


def host(r, sol=None, rows=None, idx=None):
    from mpc_ros_amd import solver

    idx = slice(None) if idx is None else idx
    return solver.sens(dict(r["P"]), r["state"][idx], r["coeffs"][idx], r["sol"][idx] if sol is None else sol,
                       params_rows=rows, want_dx=True)


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_the_host_entry(torch_cuda, name):  # noqa: F811
    r = solved(torch_cuda, name)
    h = host(r)
    np.testing.assert_array_equal(r["info"], h["info"])
    ok = h["info"] == 0
    assert ok.any() and (r["status"][ok] == 1).any()
    assert np.isnan(r["gain"][~ok]).all() and np.isnan(r["dx"][~ok]).all()
    e = rel_err(r["gain"][ok], r["dx"][ok], h["gain"][ok], h["dx"][ok])
    print(f"{name}: {ok.sum()} of {len(ok)} rows valid, max |G| {np.abs(h['gain'][ok]).max():.3e}, "
          f"device against host max |delta| / max(1, max|G|) = {e.max():.3e} (bound {SENS_DEVICE_BOUND:.1e})")
    assert (e <= SENS_DEVICE_BOUND).all()
    N = r["N"]
    np.testing.assert_array_equal(r["dx"][ok][:, :, [6 * N, 7 * N - 1]].transpose(0, 2, 1), r["gain"][ok])
    # without dx: the same gain
    g = solve_and_sens(torch_cuda, r["solver"], r["state"], r["coeffs"], sol_in=r["sol"], want_dx=False)
    np.testing.assert_array_equal(g["gain"], r["gain"])
    np.testing.assert_array_equal(g["info"], r["info"])


def test_kernel_against_the_dense_solve(torch_cuda, oracle):  # noqa: F811
    r = solved(torch_cuda, "infinity")
    N = r["N"]
    assert (r["status"][:8] == 1).all() and (r["info"][:8] == 0).all()
    ref = [dense_reference(oracle, r["P"], r["coeffs"][b], r["sol"][b]) for b in range(8)]
    assert all(i == (8 * N - 2, 6 * N) for _, _, i in ref)
    e = rel_err(r["gain"][:8], r["dx"][:8], np.array([g for g, _, _ in ref]), np.array([d for _, d, _ in ref]))
    print(f"infinity rows 0..7: device against dense max |delta| / max(1, max|G|) = {e.max():.3e}")
    assert (e <= SENS_DENSE_BOUND).all()


def test_flag_records_in_one_batch(torch_cuda, oracle, tmp_path_factory):  # noqa: F811
    """The four flag records of the host test between good rows: their flags, NaN, and the
    neighbours' bits unchanged."""
    hr = records("infinity", oracle, tmp_path_factory)
    sols, rows, want = flag_records(hr)
    idx = [0, 1, 1, 1, 1, 2]
    batch = np.concatenate([hr["sol"][[0]], sols, hr["sol"][[2]]])
    all_rows = np.concatenate([rows[[0]], rows, rows[[0]]])
    s = solver_for(hr["P"])
    st, cf = hr["state"][idx], hr["coeffs"][idx]
    got = solve_and_sens(torch_cuda, s, st, cf, sol_in=batch, rows=all_rows)
    np.testing.assert_array_equal(got["info"], np.r_[0, want, 0])
    assert np.isnan(got["gain"][1:5]).all() and np.isnan(got["dx"][1:5]).all()
    good = solve_and_sens(torch_cuda, s, st[[0, 5]], cf[[0, 5]], sol_in=batch[[0, 5]])
    assert (good["info"] == 0).all()
    np.testing.assert_array_equal(got["gain"][[0, 5]], good["gain"])
    np.testing.assert_array_equal(got["dx"][[0, 5]], good["dx"])


def test_the_correction_equals_the_host_rule(torch_cuda):  # noqa: F811
    torch = torch_cuda
    from mpc_ros_amd import solver

    r = solved(torch, "infinity")
    g, u0, ds, dc, rows = apply_case(r, r["gain"][:12])
    for kw in (dict(dcoeffs=dc), dict(), dict(dcoeffs=dc, rows=rows)):
        u = torch.full((12, 2), 7.0, dtype=torch.float64, device="cuda:0")
        r["solver"].sens_apply_device(dev(torch, g), dev(torch, u0), dev(torch, ds), u,
                                      dcoeffs=dev(torch, kw["dcoeffs"]) if "dcoeffs" in kw else None,
                                      pparams=dev(torch, kw["rows"]) if "rows" in kw else None)
        torch.cuda.synchronize()
        want = solver.sens_apply(dict(r["P"]), g, u0, ds, dcoeffs=kw.get("dcoeffs"), params_rows=kw.get("rows"))
        np.testing.assert_array_equal(u.cpu().numpy(), want)
        np.testing.assert_array_equal(want, apply_rule(r["P"], g, u0, ds, **kw))


def test_solve_gain_and_correction_in_one_graph(torch_cuda):  # noqa: F811
    """One capture of the solve with the record, the sensitivities of that record and the
    correction, replayed twice: the bytes of the direct calls."""
    torch = torch_cuda
    from mpc_ros_amd.solver import solution_elems

    r = solved(torch, "infinity")
    B, N = len(r["state"]), r["N"]
    d = torch.device("cuda:0")
    s = solver_for(r["P"])
    s.reserve(B)
    st, cf = dev(torch, r["state"]), dev(torch, r["coeffs"])
    _, _, ds, dc, _ = apply_case(r, r["gain"])
    tds, tdc = dev(torch, ds), dev(torch, dc)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=d)
    sol = torch.empty((B, solution_elems(N)), dtype=torch.float64, device=d)
    gain = torch.empty((B, 2, 10), dtype=torch.float64, device=d)
    dx = torch.empty((B, 10, 8 * N - 2), dtype=torch.float64, device=d)
    info = torch.empty(B, dtype=torch.int32, device=d)
    u = torch.empty((B, 2), dtype=torch.float64, device=d)
    outs = (u0, sol, gain, dx, info, u)

    def chain():
        s.solve_device(st, cf, u0, sol=sol)
        s.sens_device(st, cf, sol, gain, dx=dx, info=info)
        s.sens_apply_device(gain, u0, tds, u, dcoeffs=tdc)

    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        chain()  # (warm-up on the capture stream; the direct calls' bytes)
    torch.cuda.synchronize()
    ref = [t.cpu().numpy().copy() for t in outs]
    np.testing.assert_array_equal(ref[2], r["gain"])
    np.testing.assert_array_equal(ref[3], r["dx"])
    assert not np.array_equal(ref[5], ref[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain()
    for _ in range(2):
        for t in outs:
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for t, a in zip(outs, ref):
            np.testing.assert_array_equal(t.cpu().numpy(), a)


def test_host_solve_returns_the_gain(torch_cuda):  # noqa: F811
    r = solved(torch_cuda, "infinity")
    out = r["solver"].solve(r["state"][:4], r["coeffs"][:4], want_solution=True, want_gain=True)
    np.testing.assert_array_equal(out["sol"], r["sol"][:4])
    h = host(r, idx=slice(0, 4))
    np.testing.assert_array_equal(out["gain"], h["gain"])
    np.testing.assert_array_equal(out["sens_info"], h["info"])


def test_refused_before_any_launch(torch_cuda):  # noqa: F811
    import ctypes as C

    torch = torch_cuda
    from mpc_ros_amd import _lib, params

    r = solved(torch, "infinity")
    L, s = _lib.lib(), r["solver"]
    st, cf, sol = dev(torch, r["state"]), dev(torch, r["coeffs"]), dev(torch, r["sol"])
    gain = torch.zeros((len(r["state"]), 2, 10), dtype=torch.float64, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    B = len(r["state"])
    assert L.mpcg_sens_device(s._h, B, p(st), p(cf), None, None, p(gain), None, None, None) == -1
    assert L.mpcg_sens_device(s._h, B, p(st), p(cf), None, p(sol), None, None, None, None) == -1
    f32 = solver_for(r["P"], dtype="fp32")
    rows = dev(torch, params.rows(r["P"], B))
    assert L.mpcg_sens_device(f32._h, B, p(st), p(cf), p(rows), p(sol), p(gain), None, None, None) == -1
    assert "fp32" in L.mpcg_last_error().decode()


def test_cpp_class_feedback_gain(torch_cuda, tmp_path, infinity_golden):  # noqa: F811
    """MPC::feedback_gain() through a small C++ caller equals mpcg_sens on the class's own record."""
    from mpc_ros_amd import solver
    from mpc_ros_amd.params import PLUGIN_DEFAULTS

    exe = str(tmp_path / "mpc_gain")
    lib = os.path.join(ROOT, "mpc_ros_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "mpc_gain_check.cpp"), "-L", lib, "-lmpcg",
                           "-L/opt/rocm/lib", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    g = infinity_golden
    rows = (0, 1, 2)
    lines = [" ".join(repr(float(v)) for v in np.concatenate([g["state"][b], g["coeffs"][b]])) for b in rows]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                         check=True).stdout.strip().split("\n")
    assert len(out) == len(rows)
    for line, b in zip(out, rows):
        vals = np.array(line.split(), dtype=float)
        u0, info, gain, sol = vals[:2], int(vals[2]), vals[3:23].reshape(2, 10), vals[23:]
        np.testing.assert_array_equal(u0, sol[[6 * 20, 7 * 20 - 1]])
        h = solver.sens(dict(PLUGIN_DEFAULTS), g["state"][[b]], g["coeffs"][[b]], sol[None])
        assert info == 0 and h["info"][0] == 0
        np.testing.assert_array_equal(gain, h["gain"][0])
