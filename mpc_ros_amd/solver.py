"""Batched NMPC solver on one MI355X (wrapper of the C-ABI in include/mpcg.h).

``BatchSolver`` owns one ``mpcg_handle`` (one GPU).  ``solve`` takes host numpy
arrays; ``solve_device`` takes torch tensors already resident in HBM and queues
the kernel on the current torch stream without any host synchronisation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .params import PLUGIN_DEFAULTS

# The Ipopt options of the reference's solve (mpc_planner.cpp:356-368: max_cpu_time 0.5, the rest
# Ipopt 3.12 defaults) are the library's defaults (mpcg_params_default / _plugin_default); any
# mpcg_params field can be overridden by keyword.

# the fp32 configuration (precision 1, BASELINE configs[2]) runs two phases (mpcg_wide.hip):
# (1) the fp32 solver on the whole batch with tolerances a float iterate can meet -- the scaled
#     dual infeasibility of an fp32 iterate stalls near 1e-4 (multipliers ~1e3 times
#     FLT_EPSILON) and mu_min = min(tol, compl_inf_tol) / 11 must stay above float resolution;
#     it stops at tol 1e-3 (acceptable termination at 1e-3 and a 300-iteration cap end stalls);
# (2) the fp64 solver with the reference's Ipopt options on the whole batch again: from the fp32
#     iterate where the fp32 solve converged (status 1 or 4: a few fp64 iterations to Ipopt's
#     tolerance, diag[:, 2] == 4), else from the start (its line search failed at a float
#     iterate's noise floor where Ipopt would enter the restoration phase, a tiny step, the
#     iteration limit: diag[:, 2] == 3, bitwise the fp64 solver's result).
# (B > 2048: the B / 1024 problems the solve order ranks longest are solved by the fp64 solver from
# the start, diag[:, 2] == 3, while the fp32 phase runs the others.)
# The returned controls are the fp64 solver's (within 1e-6 of the reference's double-precision
# solve where they converge to the same local minimum).  no_restoration = 1 runs the fp32 phase
# alone and keeps its ending (status 9, 3 or 2 where it cannot finish).
FP32_OPTIONS = dict(precision=1, tol=1e-3, compl_inf_tol=1e-2, tiny_step_tol=10 * 1.1920928955078125e-07,
                    acceptable_tol=1e-3, max_iter=300, no_restoration=0)


def _params_struct(params, dtype, ipopt, base="plugin"):
    """mpcg_params: the base's defaults ("plugin": PLUGIN_DEFAULTS' values, "class": MPC::MPC's),
    the parameter map if any, then the keywords by field name (dtype "fp32": FP32_OPTIONS first)."""
    if dtype == "fp32":
        ipopt = dict(FP32_OPTIONS, **ipopt)
    p = _lib.params_from_map(params if params is not None else {}, base)
    for k, v in ipopt.items():
        if not hasattr(p, k):
            raise AttributeError(f"mpcg_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _host_batch(state, coeffs, N, want_traj=True, diag=False):
    """The inputs as contiguous float64 arrays, the host output arrays of B solves by name, and
    the pointers of both in the C-ABI's argument order."""
    state = np.ascontiguousarray(state, dtype=np.float64)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    B = state.shape[0]
    assert state.shape == (B, 6) and coeffs.shape == (B, 4), "state [B,6], coeffs [B,4]"
    out = dict(u0=np.zeros((B, 2)), traj=np.zeros((B, 3, N)) if want_traj else None,
               status=np.zeros(B, dtype=np.int32), obj=np.zeros(B), iters=np.zeros(B, dtype=np.int32))
    if diag:
        out["diag"] = np.zeros((B, 4), dtype=np.int32)
    ptrs = [a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double)) if a is not None else None
            for a in (state, coeffs, *out.values())]
    return B, out, ptrs


def solution_elems(N: int) -> int:
    """Doubles of one problem's solution record (mpcg_solution_elems): 3 (8N - 2) + 6N."""
    return 3 * (8 * N - 2) + 6 * N


def split_solution(sol, N: int) -> dict:
    """Views of the records sol [..., solution_elems(N)] (numpy or torch): x, zl, zu [..., 8N-2] in
    the reference's vars order and lam [..., 6N] in FG_eval's row order (include/mpcg.h)."""
    nx = 8 * N - 2
    assert sol.shape[-1] == solution_elems(N), "sol [..., 3 (8N - 2) + 6N]"
    return dict(x=sol[..., :nx], zl=sol[..., nx:2 * nx], zu=sol[..., 2 * nx:3 * nx], lam=sol[..., 3 * nx:])


def kkt(params, state, coeffs, sol, params_rows=None, base: str = "plugin", **ipopt) -> np.ndarray:
    """The KKT certificate of the records sol on the host (mpcg_kkt: no GPU, no handle): cert [B, 4]
    = stationarity, primal violation, complementarity (all unscaled, against MPC::Solve's own
    bounds) and the objective.  params: a parameter map or an mpcg_params struct."""
    p = params if isinstance(params, _lib.MpcgParams) else _params_struct(params, "fp64", ipopt, base)
    state = np.ascontiguousarray(state, dtype=np.float64)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    sol = np.ascontiguousarray(sol, dtype=np.float64)
    B = state.shape[0]
    assert state.shape == (B, 6) and coeffs.shape == (B, 4) and sol.shape == (B, solution_elems(p.steps))
    dp = C.POINTER(C.c_double)
    rows = None
    if params_rows is not None:
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
    cert = np.zeros((B, 4))
    _lib.check(_lib.lib().mpcg_kkt(C.byref(p), B, state.ctypes.data_as(dp), coeffs.ctypes.data_as(dp),
                                   rows.ctypes.data_as(dp) if rows is not None else None, sol.ctypes.data_as(dp),
                                   cert.ctypes.data_as(dp)), "mpcg_kkt")
    return cert


def sens(params, state, coeffs, sol, params_rows=None, want_dx: bool = False, base: str = "plugin", **ipopt) -> dict:
    """The feedback gains of the records sol on the host (mpcg_sens: no GPU, no handle): "gain"
    [B, 2, 10] = d(omega_0, a_0) / d(state, coeffs), "info" [B] int32 (0 valid, 1 wrong inertia, 2
    invalid row or record; gain is NaN for 1 and 2) and, with want_dx, "dx" [B, 10, 8N-2], the full
    primal columns.  params: a parameter map or an mpcg_params struct (constr_viol_tol and
    bound_relax_factor are the relaxation of the slacks)."""
    p = params if isinstance(params, _lib.MpcgParams) else _params_struct(params, "fp64", ipopt, base)
    state = np.ascontiguousarray(state, dtype=np.float64)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    sol = np.ascontiguousarray(sol, dtype=np.float64)
    B = state.shape[0]
    assert state.shape == (B, 6) and coeffs.shape == (B, 4) and sol.shape == (B, solution_elems(p.steps))
    dp = C.POINTER(C.c_double)
    rows = None
    if params_rows is not None:
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
    out = dict(gain=np.zeros((B, 2, _lib.SENS_COLS)), info=np.zeros(B, dtype=np.int32))
    if want_dx:
        out["dx"] = np.zeros((B, _lib.SENS_COLS, 8 * p.steps - 2))
    _lib.check(_lib.lib().mpcg_sens(C.byref(p), B, state.ctypes.data_as(dp), coeffs.ctypes.data_as(dp),
                                    rows.ctypes.data_as(dp) if rows is not None else None, sol.ctypes.data_as(dp),
                                    out["gain"].ctypes.data_as(dp), out["dx"].ctypes.data_as(dp) if want_dx else None,
                                    out["info"].ctypes.data_as(C.POINTER(C.c_int32))), "mpcg_sens")
    return out


def sens_apply(params, gain, u0, dstate, dcoeffs=None, params_rows=None, base: str = "plugin", **ipopt) -> np.ndarray:
    """The correction rule on the host (mpcg_sens_apply): u [B, 2] = clip(u0 + gain [dstate;
    dcoeffs]) to the handle's (or the row's) ANGVEL and MAXTHR; a NaN gain gives u0."""
    p = params if isinstance(params, _lib.MpcgParams) else _params_struct(params, "fp64", ipopt, base)
    dp = C.POINTER(C.c_double)
    gain, u0, dstate = (np.ascontiguousarray(a, dtype=np.float64) for a in (gain, u0, dstate))
    B = u0.shape[0]
    assert gain.shape == (B, 2, _lib.SENS_COLS) and u0.shape == (B, 2) and dstate.shape == (B, 6)
    dc = rows = None
    if dcoeffs is not None:
        dc = np.ascontiguousarray(dcoeffs, dtype=np.float64)
        assert dc.shape == (B, 4)
    if params_rows is not None:
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
    u = np.zeros((B, 2))
    _lib.check(_lib.lib().mpcg_sens_apply(C.byref(p), B, rows.ctypes.data_as(dp) if rows is not None else None,
                                          gain.ctypes.data_as(dp), u0.ctypes.data_as(dp), dstate.ctypes.data_as(dp),
                                          dc.ctypes.data_as(dp) if dc is not None else None, u.ctypes.data_as(dp)),
               "mpcg_sens_apply")
    return u


def shift_solution(params, state, coeffs, motion, sol, mask=None, params_rows=None, out=None, base: str = "plugin",
                   **ipopt) -> np.ndarray:
    """The records sol [B, solution_elems(N)] carried to the next tick on the host (mpcg_shift_solution:
    no GPU, no handle): shifted by one stage and moved to the frame motion [B, 3] = (mx, my, mpsi) --
    the new frame's origin and heading in the old frame -- towards the new problems state [B, 6],
    coeffs [B, 4] (params_rows [B, 16]: their parameter rows).  mask [B] int32: 0 copies the record
    unchanged.  out: the array written (it may be sol itself); a new one by default.  params: a
    parameter map or an mpcg_params struct."""
    p = params if isinstance(params, _lib.MpcgParams) else _params_struct(params, "fp64", ipopt, base)
    state = np.ascontiguousarray(state, dtype=np.float64)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    motion = np.ascontiguousarray(motion, dtype=np.float64)
    B = state.shape[0]
    ne = solution_elems(p.steps)
    if out is not sol:
        sol = np.ascontiguousarray(sol, dtype=np.float64)
    assert state.shape == (B, 6) and coeffs.shape == (B, 4) and motion.shape == (B, 3) and sol.shape == (B, ne)
    assert sol.dtype == np.float64 and sol.flags.c_contiguous
    if out is None:
        out = np.empty((B, ne))
    assert out.shape == (B, ne) and out.dtype == np.float64 and out.flags.c_contiguous
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rows = m = None
    if params_rows is not None:
        rows = np.ascontiguousarray(params_rows, dtype=np.float64)
        assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.int32)
        assert m.shape == (B,)
    _lib.check(_lib.lib().mpcg_shift_solution(
        C.byref(p), B, state.ctypes.data_as(dp), coeffs.ctypes.data_as(dp),
        rows.ctypes.data_as(dp) if rows is not None else None, motion.ctypes.data_as(dp),
        m.ctypes.data_as(ip) if m is not None else None, sol.ctypes.data_as(dp), out.ctypes.data_as(dp)),
        "mpcg_shift_solution")
    return out


def _on_device(t, shape, dtype="float64"):
    """t is a contiguous torch tensor of this dtype and shape on a GPU."""
    import torch

    assert t.is_cuda and t.dtype == getattr(torch, dtype) and t.is_contiguous() and tuple(t.shape) == tuple(shape)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(stream, like):
    """The stream's handle for the C-ABI (None: torch's current stream on `like`'s device)."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream(like.device)
    return C.c_void_p(stream.cuda_stream)


class BatchSolver:
    def __init__(self, device: int = 0, params: dict | None = None, strategy: str = "wave", dtype: str = "fp64",
                 **ipopt):
        """dtype "fp32": the fp32 solver with FP32_OPTIONS (overridable by keyword)."""
        if dtype == "fp32":
            ipopt = dict(FP32_OPTIONS, **ipopt)
        elif dtype != "fp64":
            raise ValueError("dtype must be 'fp64' or 'fp32'")
        L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.mpcg_create(int(device), C.byref(h)), "mpcg_create")
        self._h = h
        self.device = device
        self.set_params(params if params is not None else PLUGIN_DEFAULTS, **ipopt)
        self.set_strategy(strategy)

    def set_strategy(self, strategy: str = "wave"):
        """'wave' (= 'auto'): one problem per wavefront, LDS-resident (the only kernel strategy)."""
        _lib.check(_lib.lib().mpcg_set_strategy(self._h, _lib.STRATEGY[strategy]), "mpcg_set_strategy")

    @property
    def strategy(self) -> str:
        v = _lib.lib().mpcg_get_strategy(self._h)
        return {v2: k for k, v2 in _lib.STRATEGY.items()}[v]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mpcg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ parameters
    def set_params(self, params: dict, base: str = "plugin", **ipopt):
        p = _params_struct(params, "fp64", ipopt, base)
        _lib.check(_lib.lib().mpcg_set_params(self._h, C.byref(p)), "mpcg_set_params")
        self.params = p
        self.N = p.steps

    def set_park_capacity(self, cap: int = 0):
        """Park-area entries (0: the default max(256, B / 128)); results do not depend on it."""
        _lib.check(_lib.lib().mpcg_set_park_capacity(self._h, int(cap)), "mpcg_set_park_capacity")

    @property
    def last_kernel(self) -> str:
        """The solver kernel instance the last solve launched ("k_solve_wide<...>")."""
        return _lib.lib().mpcg_last_kernel(self._h).decode()

    @property
    def last_solve_order(self) -> bool:
        """True if the last solve ran its problems expected-longest first (B > 2048)."""
        return bool(_lib.lib().mpcg_last_solve_order(self._h))

    def reserve(self, B: int):
        _lib.check(_lib.lib().mpcg_reserve(self._h, int(B)), "mpcg_reserve")

    def workspace_bytes(self, B: int) -> int:
        """What reserve(B) allocates (the handle's park capacity and device included)."""
        return int(_lib.lib().mpcg_handle_workspace_bytes(self._h, int(B)))

    # ----------------------------------------------------------------- solve
    def solve(self, state: np.ndarray, coeffs: np.ndarray, want_traj: bool = True, params_rows=None,
              want_solution: bool = False, want_gain: bool = False, start=None, start_mode=None,
              mu0=None) -> dict:
        """params_rows [B, 16] (params.rows): a parameter row per problem instead of the handle's
        per-problem fields (mpcg_solve_pp); a row outside the parameters' domains raises.
        want_solution: also the full solution (mpcg_solve_sol) -- "sol" [B, solution_elems(N)] and
        its views "x", "zl", "zu" [B, 8N-2] and "lam" [B, 6N] (split_solution).
        want_gain (with want_solution): also the feedback gains of the records (mpcg_sens) -- "gain"
        [B, 2, 10] and "sens_info" [B].
        start [B, solution_elems(N)] with start_mode (an int, or [B] int32: _lib.START_COLD / _PRIMAL /
        _FULL per problem) and mu0 (None: mu_init; a float or [B], read in FULL mode): the solve
        started from the records (mpcg_solve_start); the result then has "start_used" [B], the mode
        that ran (negative: the start was not usable and the problem was solved cold)."""
        if start is not None:
            return self._solve_start(state, coeffs, want_traj, params_rows, want_solution, want_gain, start,
                                     start_mode, mu0)
        if start_mode is not None or mu0 is not None:
            raise ValueError("start_mode and mu0 need start")
        if want_gain and not want_solution:
            raise ValueError("want_gain needs want_solution: the gain is computed from the record")
        B, out, ptrs = _host_batch(state, coeffs, self.N, want_traj, diag=True)
        rows = None
        if params_rows is not None:
            rows = np.ascontiguousarray(params_rows, dtype=np.float64)
            assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
        if want_solution:
            dp = C.POINTER(C.c_double)
            sol = np.zeros((B, solution_elems(self.N)))
            _lib.check(_lib.lib().mpcg_solve_sol(self._h, B, ptrs[0], ptrs[1],
                                                 rows.ctypes.data_as(dp) if rows is not None else None, *ptrs[2:],
                                                 sol.ctypes.data_as(dp)), "mpcg_solve_sol")
            out["sol"] = sol
            out.update(split_solution(sol, self.N))
            if want_gain:
                g = sens(self.params, state, coeffs, sol, params_rows=rows)
                out["gain"], out["sens_info"] = g["gain"], g["info"]
            return out
        if params_rows is not None:
            _lib.check(_lib.lib().mpcg_solve_pp(self._h, B, ptrs[0], ptrs[1], rows.ctypes.data_as(C.POINTER(C.c_double)),
                                                *ptrs[2:]), "mpcg_solve_pp")
            return out
        _lib.check(_lib.lib().mpcg_solve_ex(self._h, B, *ptrs), "mpcg_solve_ex")
        # diag columns: restoration phases, filter entries dropped beyond its capacity, parked,
        # most filter entries held at once
        return out

    def _solve_start(self, state, coeffs, want_traj, params_rows, want_solution, want_gain, start, start_mode, mu0):
        if want_gain and not want_solution:
            raise ValueError("want_gain needs want_solution: the gain is computed from the record")
        if start_mode is None:
            raise ValueError("start needs start_mode")
        B, out, ptrs = _host_batch(state, coeffs, self.N, want_traj, diag=True)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        rows = None
        if params_rows is not None:
            rows = np.ascontiguousarray(params_rows, dtype=np.float64)
            assert rows.shape == (B, _lib.PP_FIELDS), "params_rows [B,16]"
        start = np.ascontiguousarray(start, dtype=np.float64)
        assert start.shape == (B, solution_elems(self.N)), "start [B, solution_elems(N)]"
        mode = np.ascontiguousarray(np.broadcast_to(np.asarray(start_mode, dtype=np.int32), (B,)))
        m0 = None if mu0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mu0, dtype=np.float64), (B,)))
        sol = np.zeros((B, solution_elems(self.N))) if want_solution else None
        used = np.zeros(B, dtype=np.int32)
        _lib.check(_lib.lib().mpcg_solve_start(
            self._h, B, ptrs[0], ptrs[1], rows.ctypes.data_as(dp) if rows is not None else None,
            start.ctypes.data_as(dp), mode.ctypes.data_as(ip), m0.ctypes.data_as(dp) if m0 is not None else None,
            *ptrs[2:], sol.ctypes.data_as(dp) if sol is not None else None, used.ctypes.data_as(ip)),
            "mpcg_solve_start")
        out["start_used"] = used
        if want_solution:
            out["sol"] = sol
            out.update(split_solution(sol, self.N))
            if want_gain:
                g = sens(self.params, state, coeffs, sol, params_rows=rows)
                out["gain"], out["sens_info"] = g["gain"], g["info"]
        return out

    def solve_device(self, state, coeffs, u0, traj=None, status=None, obj=None, iters=None, stream=None, diag=None,
                     pparams=None, sol=None, start=None, start_mode=None, mu0=None, start_used=None):
        """All arguments are torch tensors on this handle's GPU (float64 / int32, contiguous);
        diag [B, 4] int32: restoration phases, filter overflows, parked, filter peak.
        pparams [B, 16] float64: a parameter row per problem (mpcg_solve_device_pp), read when the
        stream runs the solve -- keep it unchanged until then.  A row outside the parameters'
        domains ends its problem with status 13, iters 0 and zero outputs.
        sol [B, solution_elems(N)] float64: the full solution records (mpcg_solve_device_sol).
        start [B, solution_elems(N)] float64 with start_mode [B] int32 (an int broadcasts: a tensor
        is made), mu0 [B] float64 or None and start_used [B] int32 or None: the solve started from the
        records (mpcg_solve_device_start); sol may be None and may be the start tensor itself (the
        in-place loop).  start, start_mode and mu0 are read when the stream runs the solve."""
        import torch

        B = state.shape[0]
        for t, shape in ((state, (B, 6)), (coeffs, (B, 4)), (u0, (B, 2))):
            _on_device(t, shape)
        if traj is not None:
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.numel() == B * 3 * self.N
        for t in (status, iters):
            assert t is None or (t.dtype == torch.int32 and t.numel() == B)
        assert diag is None or (diag.dtype == torch.int32 and diag.numel() == 4 * B and diag.is_contiguous())
        ptr, sp = _ptr, _stream_ptr(stream, state)
        if pparams is not None:
            _on_device(pparams, (B, _lib.PP_FIELDS))
        if start is not None:
            if start_mode is None:
                raise ValueError("start needs start_mode")
            if not torch.is_tensor(start_mode):
                start_mode = torch.full((B,), int(start_mode), dtype=torch.int32, device=state.device)
            _on_device(start, (B, solution_elems(self.N)))
            _on_device(start_mode, (B,), "int32")
            if mu0 is not None:
                _on_device(mu0, (B,))
            if start_used is not None:
                _on_device(start_used, (B,), "int32")
            if sol is not None:
                _on_device(sol, (B, solution_elems(self.N)))
            _lib.check(_lib.lib().mpcg_solve_device_start(
                self._h, B, ptr(state), ptr(coeffs), ptr(pparams), ptr(start), ptr(start_mode), ptr(mu0), ptr(u0),
                ptr(traj), ptr(status), ptr(obj), ptr(iters), ptr(diag), ptr(sol), ptr(start_used), sp),
                "mpcg_solve_device_start")
            return
        if start_mode is not None or mu0 is not None or start_used is not None:
            raise ValueError("start_mode, mu0 and start_used need start")
        if sol is not None:
            _on_device(sol, (B, solution_elems(self.N)))
            _lib.check(_lib.lib().mpcg_solve_device_sol(
                self._h, B, ptr(state), ptr(coeffs), ptr(pparams), ptr(u0), ptr(traj), ptr(status), ptr(obj),
                ptr(iters), ptr(diag), ptr(sol), sp), "mpcg_solve_device_sol")
            return
        if pparams is not None:
            _lib.check(_lib.lib().mpcg_solve_device_pp(
                self._h, B, ptr(state), ptr(coeffs), ptr(pparams), ptr(u0), ptr(traj), ptr(status), ptr(obj),
                ptr(iters), ptr(diag), sp), "mpcg_solve_device_pp")
            return
        _lib.check(_lib.lib().mpcg_solve_device_ex(
            self._h, B, ptr(state), ptr(coeffs), ptr(u0), ptr(traj), ptr(status), ptr(obj), ptr(iters), ptr(diag),
            sp), "mpcg_solve_device_ex")

    def kkt_device(self, state, coeffs, sol, cert, pparams=None, stream=None):
        """The KKT certificate of the records sol [B, solution_elems(N)] on the device
        (mpcg_kkt_device): cert [B, 4] float64 = stationarity, primal violation, complementarity,
        objective; the handle's parameters, or a row per problem (pparams [B, 16]; an invalid row
        gives NaN).  Queued on the stream, no allocation."""
        B = state.shape[0]
        for t, shape in ((state, (B, 6)), (coeffs, (B, 4)), (sol, (B, solution_elems(self.N))), (cert, (B, 4))):
            _on_device(t, shape)
        if pparams is not None:
            _on_device(pparams, (B, _lib.PP_FIELDS))
        _lib.check(_lib.lib().mpcg_kkt_device(self._h, B, _ptr(state), _ptr(coeffs), _ptr(pparams), _ptr(sol),
                                              _ptr(cert), _stream_ptr(stream, state)), "mpcg_kkt_device")

    def shift_solution_device(self, state, coeffs, motion, sol_in, sol_out, mask=None, pparams=None, stream=None):
        """The records sol_in [B, solution_elems(N)] carried to the next tick on the device
        (mpcg_shift_solution_device; the rule: shift_solution): motion [B, 3] float64, mask [B] int32
        or None, the new problems' state, coeffs and pparams [B, 16] (None: the handle's parameters);
        sol_out may be sol_in.  Queued on the stream, no allocation."""
        B = state.shape[0]
        ne = solution_elems(self.N)
        for t, shape in ((state, (B, 6)), (coeffs, (B, 4)), (motion, (B, 3)), (sol_in, (B, ne)), (sol_out, (B, ne))):
            _on_device(t, shape)
        if mask is not None:
            _on_device(mask, (B,), "int32")
        if pparams is not None:
            _on_device(pparams, (B, _lib.PP_FIELDS))
        _lib.check(_lib.lib().mpcg_shift_solution_device(
            self._h, B, _ptr(state), _ptr(coeffs), _ptr(pparams), _ptr(motion), _ptr(mask), _ptr(sol_in),
            _ptr(sol_out), _stream_ptr(stream, state)), "mpcg_shift_solution_device")

    def sens_device(self, state, coeffs, sol, gain, dx=None, info=None, pparams=None, stream=None):
        """The feedback gains of the records sol [B, solution_elems(N)] on the device
        (mpcg_sens_device): gain [B, 2, 10] float64, dx [B, 10, 8N-2] float64 and info [B] int32
        (both optional); the handle's parameters, or a row per problem (pparams [B, 16]).  Queued on
        the stream, no allocation."""
        B = state.shape[0]
        for t, shape in ((state, (B, 6)), (coeffs, (B, 4)), (sol, (B, solution_elems(self.N))),
                         (gain, (B, 2, _lib.SENS_COLS))):
            _on_device(t, shape)
        if dx is not None:
            _on_device(dx, (B, _lib.SENS_COLS, 8 * self.N - 2))
        if info is not None:
            _on_device(info, (B,), "int32")
        if pparams is not None:
            _on_device(pparams, (B, _lib.PP_FIELDS))
        _lib.check(_lib.lib().mpcg_sens_device(self._h, B, _ptr(state), _ptr(coeffs), _ptr(pparams), _ptr(sol),
                                               _ptr(gain), _ptr(dx), _ptr(info), _stream_ptr(stream, state)),
                   "mpcg_sens_device")

    def sens_apply_device(self, gain, u0, dstate, u, dcoeffs=None, pparams=None, stream=None):
        """u [B, 2] = clip(u0 + gain [dstate; dcoeffs]) on the device (mpcg_sens_apply_device), one
        robot per lane: the correction of a delay-mode prediction without a solve.  dcoeffs [B, 4]
        or None (0); the limits are the handle's, or the row's (pparams [B, 16])."""
        B = u0.shape[0]
        for t, shape in ((gain, (B, 2, _lib.SENS_COLS)), (u0, (B, 2)), (dstate, (B, 6)), (u, (B, 2))):
            _on_device(t, shape)
        if dcoeffs is not None:
            _on_device(dcoeffs, (B, 4))
        if pparams is not None:
            _on_device(pparams, (B, _lib.PP_FIELDS))
        _lib.check(_lib.lib().mpcg_sens_apply_device(self._h, B, _ptr(pparams), _ptr(gain), _ptr(u0), _ptr(dstate),
                                                     _ptr(dcoeffs), _ptr(u), _stream_ptr(stream, u0)),
                   "mpcg_sens_apply_device")

    # ------------------------------------------------ the benchmark's synthetic robots
    def synth_infinity_device(self, start: int, B: int, M: int = 11, seed: int | None = None, stream=None):
        """Robots start .. start + B - 1 of the infinity set generated on this GPU from (seed,
        global index) (mpcg_synth_infinity_device): torch tensors pose [B,3], vel [B,3], plan [B,M,2]."""
        import torch

        from . import infinity

        dev = torch.device("cuda", self.device)
        pose = torch.empty((B, 3), dtype=torch.float64, device=dev)
        vel = torch.empty((B, 3), dtype=torch.float64, device=dev)
        plan = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().mpcg_synth_infinity_device(
            self._h, int(infinity.SEED if seed is None else seed), int(start), int(B), int(M), _ptr(pose), _ptr(vel),
            _ptr(plan), _stream_ptr(stream, pose)), "mpcg_synth_infinity_device")
        return pose, vel, plan

    # ------------------------------------------------ the caller side on the device
    def preprocess_device(self, pose, vel, plan, state, coeffs, delay_mode: bool = True, stream=None, count=None):
        """Tracking::findBestPath's preprocessing (driving_state.cpp:175-256) for B robots.

        pose [B,3] (x, y, yaw), vel [B,3] (v feedback, previous w, previous throttle),
        plan [B,M,2] -> state [B,6], coeffs [B,4]; torch float64 tensors on this GPU.
        count [B] int32: robot p's own waypoint count in its M <= 64 plan rows
        (mpcg_preprocess_device_n); a robot with count < 4 is not fitted, its outputs are 0."""
        B, M = plan.shape[0], plan.shape[1]
        for t, shape in ((pose, (B, 3)), (vel, (B, 3)), (plan, (B, M, 2)), (state, (B, 6)), (coeffs, (B, 4))):
            _on_device(t, shape)
        ptr, sp = _ptr, _stream_ptr(stream, pose)
        if count is not None:
            _on_device(count, (B,), "int32")
            _lib.check(_lib.lib().mpcg_preprocess_device_n(
                self._h, B, M, ptr(pose), ptr(vel), ptr(plan), ptr(count), int(bool(delay_mode)), ptr(state),
                ptr(coeffs), sp), "mpcg_preprocess_device_n")
            return
        _lib.check(_lib.lib().mpcg_preprocess_device(
            self._h, B, M, ptr(pose), ptr(vel), ptr(plan), int(bool(delay_mode)), ptr(state), ptr(coeffs), sp),
            "mpcg_preprocess_device")

    def track_device(self, pose, vel, plan, cmd, traj=None, status=None, delay_mode: bool = True, stream=None,
                     goal=None, ref_v=None, max_speed: float = 0.7, min_speed: float = 0.05):
        """One control tick for B robots: preprocessing, solve, post-processing
        (driving_state.cpp:175-269).  cmd [B,3] = (speed, w, throttle).

        With goal [B,2] and ref_v [B] (in/out): the tick of mpcComputeVelocityCommands
        (mpcg_track_device_goal) -- Tracking::deceleration rewrites each robot's REF_V in ref_v
        from its distance to its goal (max_speed, min_speed: driving_state.cpp:26, :29), the
        solve and the speed clamp use it; pass ref_v back in at the next tick."""
        import torch

        B, M = plan.shape[0], plan.shape[1]
        for t, shape in ((pose, (B, 3)), (vel, (B, 3)), (plan, (B, M, 2)), (cmd, (B, 3))):
            _on_device(t, shape)
        if traj is not None:
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.numel() == B * 3 * self.N
        assert status is None or (status.dtype == torch.int32 and status.numel() == B)
        ptr, sp = _ptr, _stream_ptr(stream, pose)
        if (goal is None) != (ref_v is None):
            raise ValueError("goal and ref_v go together")
        if goal is not None:
            _on_device(goal, (B, 2))
            _on_device(ref_v, (B,))
            _lib.check(_lib.lib().mpcg_track_device_goal(
                self._h, B, M, ptr(pose), ptr(vel), ptr(plan), ptr(goal), ptr(ref_v), float(max_speed), float(min_speed),
                int(bool(delay_mode)), ptr(cmd), ptr(traj), ptr(status), sp), "mpcg_track_device_goal")
            return
        _lib.check(_lib.lib().mpcg_track_device(
            self._h, B, M, ptr(pose), ptr(vel), ptr(plan), int(bool(delay_mode)), ptr(cmd), ptr(traj), ptr(status), sp),
            "mpcg_track_device")

    # ------------------------------------------------ the closed loop on the device
    @staticmethod
    def _courses(courses, course_len, course_of, B):
        Cn, Gmax = courses.shape[0], courses.shape[1]
        _on_device(courses, (Cn, Gmax, 2))
        _on_device(course_len, (Cn,), "int32")
        _on_device(course_of, (B,), "int32")
        return Cn, Gmax

    def plan_window_device(self, courses, course_len, course_of, pose, window_wp: int, stride: int, cursor, plan,
                           count, stream=None):
        """The plan window of B robots (mpcg_plan_window_device; the rule: closed_loop.plan_window):
        courses [C,Gmax,2] float64, course_len [C] and course_of [B] int32, pose [B,3]; cursor [B]
        int32 in/out, plan [B,Mmax,2] float64 and count [B] int32 out, Mmax =
        closed_loop.plan_window_mmax(window_wp, stride)."""
        B = pose.shape[0]
        Cn, Gmax = self._courses(courses, course_len, course_of, B)
        Mmax = plan.shape[1]
        for t, shape, dt in ((pose, (B, 3), "float64"), (plan, (B, Mmax, 2), "float64"), (cursor, (B,), "int32"),
                             (count, (B,), "int32")):
            _on_device(t, shape, dt)
        want = _lib.lib().mpcg_plan_window_mmax(int(window_wp), int(stride))
        assert want < 0 or Mmax == want, f"plan must have Mmax = {want} rows per robot"
        ptr = _ptr
        _lib.check(_lib.lib().mpcg_plan_window_device(
            self._h, B, ptr(courses), ptr(course_len), ptr(course_of), Cn, Gmax, ptr(pose), int(window_wp), int(stride),
            ptr(cursor), ptr(plan), ptr(count), _stream_ptr(stream, pose)), "mpcg_plan_window_device")

    ROLLOUT_LOGS = {"pose": 3, "vel": 3, "cmd": 3, "cursor": 0, "start": 0, "count": 0, "status": 0, "iters": 0,
                    "ref_v": 0}

    @classmethod
    def _log_spec(cls, name, K, B):
        """A rollout log's shape and dtype name: the 3-wide ones and ref_v are float64, the rest int32."""
        w = cls.ROLLOUT_LOGS[name]
        return ((K, B, w) if w else (K, B)), ("float64" if w or name == "ref_v" else "int32")

    def rollout_logs(self, K: int, B: int, names=None) -> dict:
        """Log tensors for rollout(K, ..., logs=): pose, vel, cmd [K,B,3] and ref_v [K,B] float64,
        cursor, start, count, status, iters [K,B] int32 (all of them, or the names given)."""
        import torch

        dev = torch.device("cuda", self.device)
        out = {}
        for n in (names if names is not None else self.ROLLOUT_LOGS):
            shape, dt = self._log_spec(n, K, B)
            out[n] = torch.zeros(shape, dtype=getattr(torch, dt), device=dev)
        return out

    def rollout(self, K: int, courses, course_len, course_of, window_wp: int, stride: int, pose, vel, cursor, ref_v,
                done, goal_tol: float = 0.1, max_speed: float = 0.7, min_speed: float = 0.05,
                delay_mode: bool = True, integrate: bool = True, logs: dict | None = None, stream=None,
                start_mode: int = 0, mu0: float = 1e-4, carry: dict | None = None, log_start_used=None):
        """K control ticks of B robots in one enqueue (mpcg_rollout_device): per tick the plan
        window from the robot's course, deceleration towards the course's last waypoint, the
        preprocessing with the robot's own waypoint count, the solve, the post-processing and,
        with `integrate`, the unicycle of closed_loop.run.  pose [B,3], vel [B,3], ref_v [B]
        float64 and cursor [B], done [B] int32 are in/out: done[b] is the tick (index + 1) at
        which robot b stopped, at its goal (within goal_tol) or at its course's end.  logs: tensors
        by name as rollout_logs(K, B) makes them.  No host synchronisation; call it once before
        capturing it in a graph (the handle's buffers grow on first use).
        carry (rollout_carry(B); in/out like pose): every tick starts from the robot's previous
        solution (mpcg_rollout_device_start) -- start_mode _lib.START_COLD or START_FULL, the same
        for all robots (START_PRIMAL is refused), mu0 FULL's barrier parameter, log_start_used [K, B] int32 or None the mode that ran.
        A robot's record is shifted by one stage and moved to the tick's frame where it is usable
        (carry "ok", a running robot, a mode other than COLD); the others run cold."""
        B = pose.shape[0]
        Cn, Gmax = self._courses(courses, course_len, course_of, B)
        for t, shape, dt in ((pose, (B, 3), "float64"), (vel, (B, 3), "float64"), (ref_v, (B,), "float64"),
                             (cursor, (B,), "int32"), (done, (B,), "int32")):
            _on_device(t, shape, dt)
        lg = _lib.MpcgRolloutLogs()
        for n, t in (logs or {}).items():
            _on_device(t, *self._log_spec(n, K, B))
            setattr(lg, n, t.data_ptr())
        ptr = _ptr
        if carry is not None:
            _on_device(carry["sol"], (B, solution_elems(self.N)))
            _on_device(carry["pose"], (B, 3))
            _on_device(carry["ok"], (B,), "int32")
            if log_start_used is not None:
                _on_device(log_start_used, (K, B), "int32")
            _lib.check(_lib.lib().mpcg_rollout_device_start(
                self._h, B, int(K), ptr(courses), ptr(course_len), ptr(course_of), Cn, Gmax, int(window_wp),
                int(stride), float(goal_tol), float(max_speed), float(min_speed), int(bool(delay_mode)),
                int(bool(integrate)), ptr(pose), ptr(vel), ptr(cursor), ptr(ref_v), ptr(done), C.byref(lg),
                _stream_ptr(stream, pose), int(start_mode), float(mu0), ptr(carry["sol"]), ptr(carry["pose"]),
                ptr(carry["ok"]), ptr(log_start_used)), "mpcg_rollout_device_start")
            return
        if start_mode != 0 or log_start_used is not None:
            raise ValueError("start_mode and log_start_used need carry")
        _lib.check(_lib.lib().mpcg_rollout_device(
            self._h, B, int(K), ptr(courses), ptr(course_len), ptr(course_of), Cn, Gmax, int(window_wp), int(stride),
            float(goal_tol), float(max_speed), float(min_speed), int(bool(delay_mode)), int(bool(integrate)),
            ptr(pose), ptr(vel), ptr(cursor), ptr(ref_v), ptr(done), C.byref(lg), _stream_ptr(stream, pose)),
            "mpcg_rollout_device")

    def rollout_carry(self, B: int) -> dict:
        """The carry of rollout(..., carry=), zeroed: "sol" [B, solution_elems(N)] and "pose" [B, 3]
        float64, "ok" [B] int32."""
        import torch

        dev = torch.device("cuda", self.device)
        return dict(sol=torch.zeros((B, solution_elems(self.N)), dtype=torch.float64, device=dev),
                    pose=torch.zeros((B, 3), dtype=torch.float64, device=dev),
                    ok=torch.zeros(B, dtype=torch.int32, device=dev))


class MultiSolver:
    """mpcg_multi: a persistent multi-GPU context (communicator, per-GPU handles, streams and
    buffers for batches of up to B_max problems, created once); ``solve`` shards a host batch
    over the GPUs and gathers the results to devices[0] by RCCL (include/mpcg.h)."""

    def __init__(self, devices, B_max: int, params: dict | None = None, dtype: str = "fp64", **ipopt):
        self.p = _params_struct(params, dtype, ipopt)
        self.N = self.p.steps
        self.B_max = int(B_max)
        dev = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _lib.check(_lib.lib().mpcg_multi_create(len(devices), dev, C.byref(self.p), self.B_max, C.byref(h)),
                   "mpcg_multi_create")
        self._h = h

    def solve(self, state, coeffs) -> dict:
        B, out, ptrs = _host_batch(state, coeffs, self.N)
        _lib.check(_lib.lib().mpcg_multi_solve(self._h, B, *ptrs), "mpcg_multi_solve")
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mpcg_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_multi(devices, params: dict | None = None, state=None, coeffs=None, dtype: str = "fp64", **ipopt) -> dict:
    """mpcg_solve_multi: one process, the batch sharded over `devices`, results gathered to
    devices[0] by RCCL (include/mpcg.h).  Only ngpu = 1 has run on hardware (the GPU boxes
    this was developed on hold one MI355X); the shard and gather arithmetic for ngpu > 1 is
    unit-tested on the CPU (tests/test_abi.py)."""
    p = _params_struct(params, dtype, ipopt)
    B, out, ptrs = _host_batch(state, coeffs, p.steps)
    dev = (C.c_int * len(devices))(*devices)
    _lib.check(_lib.lib().mpcg_solve_multi(len(devices), dev, C.byref(p), B, *ptrs), "mpcg_solve_multi")
    return out
