"""GPU: the certificate kernel k_kkt_certify (mpcg_kkt_device) against its host mirror mpcg_kkt on
the records the GPU solver wrote.

Kernel and mirror run the same stage body without FMA contraction; they differ by the platform's
sin / cos (a few ulp) and by the order of the objective's sum (a butterfly against stage order), so
they agree to rounding, not bitwise (DESIGN.md "The full solution and its certificate"): columns
0-2 to the host test's re-evaluation tolerance 1e-11 (1 + max|grad f| + max|lambda| + max|z|) per
row, column 3 to 1e-12 relative.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import solver_for, torch_cuda  # noqa: F401
from test_gpu_solution import dev, gpu_solve, shape_cases
from test_kkt_host import push_past_bound
from test_solution_host import numpy_kkt

pytestmark = pytest.mark.gpu

SHAPES = ["N20", "N40", "N65", "bicycle_N25", "general_N20", "general_bicycle_N25"]
_solved = {}


def solved(torch, infinity_golden, name):
    """The GPU's solve of a shape's batch with the record, once; never modified."""
    if name not in _solved:
        P, st, cf = shape_cases(infinity_golden)[name]
        st, cf = np.ascontiguousarray(st[:64]), np.ascontiguousarray(cf[:64])
        s = solver_for(P)
        r = gpu_solve(torch, s, st, cf)
        r.update(P=P, N=int(P["STEPS"]), state=st, coeffs=cf, solver=s)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _solved[name] = r
    return _solved[name]


def device_cert(torch, r, sol=None, rows=None, state=None, coeffs=None):
    st = r["state"] if state is None else state
    cert = torch.full((len(st), 4), 7.0, dtype=torch.float64, device="cuda:0")
    r["solver"].kkt_device(dev(torch, st), dev(torch, r["coeffs"] if coeffs is None else coeffs),
                           dev(torch, r["sol"] if sol is None else sol), cert,
                           pparams=None if rows is None else dev(torch, rows))
    torch.cuda.synchronize()
    return cert.cpu().numpy()


def host_cert(r, sol=None, rows=None, state=None, coeffs=None):
    from mpc_ros_amd import solver

    return solver.kkt(dict(r["P"]), r["state"] if state is None else state, r["coeffs"] if coeffs is None else coeffs,
                      r["sol"] if sol is None else sol, params_rows=rows)


def scales(oracle, r, sol=None, state=None, coeffs=None):
    st, cf, so = (r["state"] if state is None else state, r["coeffs"] if coeffs is None else coeffs,
                  r["sol"] if sol is None else sol)
    return np.array([numpy_kkt(oracle, r["P"], st[b], cf[b], so[b])[1] for b in range(len(st))])


def same(dc, hc, scale):
    assert (np.abs(dc[:, :3] - hc[:, :3]).max(axis=1) <= 1e-11 * (1 + scale)).all()
    np.testing.assert_allclose(dc[:, 3], hc[:, 3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("name", SHAPES)
def test_kernel_equals_the_host_mirror(torch_cuda, oracle, infinity_golden, name, with_rows):  # noqa: F811
    from mpc_ros_amd import params

    r = solved(torch_cuda, infinity_golden, name)
    rows = None
    if with_rows:
        # the handle's own values in every row but the last, which is invalid: the kernel reads the
        # rows (NaN there) and gives the handle's certificate elsewhere
        rows = params.rows(r["P"], len(r["state"]))
        rows[-1] = 0.0
    dc, hc = device_cert(torch_cuda, r, rows=rows), host_cert(r, rows=rows)
    n = len(dc) - (1 if with_rows else 0)
    if with_rows:
        assert np.isnan(dc[-1]).all() and np.isnan(hc[-1]).all()
    sc = scales(oracle, r)
    same(dc[:n], hc[:n], sc[:n])
    ok = r["status"][:n] == 1
    assert ok.any()
    print(f"{name}: {ok.sum()} status-1 rows: dual {dc[:n][ok, 0].max():.3e} primal {dc[:n][ok, 1].max():.3e} "
          f"compl {dc[:n][ok, 2].max():.3e}")
    # the Ipopt tolerances in force (the reference's defaults), under which status 1 is returned
    assert dc[:n][ok, 0].max() <= 1.0 and dc[:n][ok, 1].max() <= 1e-4 and dc[:n][ok, 2].max() <= 1e-4
    np.testing.assert_allclose(dc[:n, 3], r["obj"][:n], rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", ["N20", "bicycle_N25"])
def test_perturbed_records_through_the_kernel(torch_cuda, oracle, infinity_golden, name):  # noqa: F811
    """The host test's perturbations: lambda of the first initial-state row + 1e-3 moves column 0 by
    1e-3 and nothing else; a control on its bound pushed 1e-3 beyond it makes column 1 1e-3."""
    r = solved(torch_cuda, infinity_golden, name)
    N, nx = r["N"], 8 * r["N"] - 2
    base = device_cert(torch_cuda, r)
    sol = r["sol"].copy()
    sol[:, 3 * nx] += 1e-3
    dc = device_cert(torch_cuda, r, sol)
    sc = scales(oracle, r, sol)
    assert (np.abs(dc[:, 0] - 1e-3) <= base[:, 0] + 1e-11 * (1 + sc)).all()
    np.testing.assert_array_equal(dc[:, 1:], base[:, 1:])
    same(dc, host_cert(r, sol), sc)
    rows, sols = push_past_bound(r)
    assert len(rows) >= 8
    st, cf = r["state"][rows], r["coeffs"][rows]
    dc = device_cert(torch_cuda, r, sols, state=st, coeffs=cf)
    np.testing.assert_allclose(dc[:, 1], 1e-3, rtol=1e-9, atol=0)
    same(dc, host_cert(r, sols, state=st, coeffs=cf), scales(oracle, r, sols, st, cf))


def test_solve_and_certificate_in_one_graph(torch_cuda, infinity_golden):  # noqa: F811
    """One capture of the solve with the record and the certificate of that record, replayed twice:
    the bytes of the direct calls."""
    torch = torch_cuda
    from mpc_ros_amd.solver import solution_elems

    r = solved(torch, infinity_golden, "N20")
    B = len(r["state"])
    d = torch.device("cuda:0")
    s = solver_for(r["P"])
    s.reserve(B)
    st, cf = dev(torch, r["state"]), dev(torch, r["coeffs"])
    u0 = torch.empty((B, 2), dtype=torch.float64, device=d)
    status = torch.empty(B, dtype=torch.int32, device=d)
    sol = torch.empty((B, solution_elems(20)), dtype=torch.float64, device=d)
    cert = torch.empty((B, 4), dtype=torch.float64, device=d)

    def both():
        s.solve_device(st, cf, u0, status=status, sol=sol)
        s.kkt_device(st, cf, sol, cert)

    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        both()  # (warm-up on the capture stream; the direct calls' bytes)
    torch.cuda.synchronize()
    ref = [t.cpu().numpy().copy() for t in (u0, status, sol, cert)]
    np.testing.assert_array_equal(ref[2], r["sol"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        both()
    for _ in range(2):
        for t in (u0, status, sol, cert):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for t, a in zip((u0, status, sol, cert), ref):
            np.testing.assert_array_equal(t.cpu().numpy(), a)
