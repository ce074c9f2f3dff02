"""GPU: a parameter row per problem in one batch (mpcg_solve_pp / mpcg_solve_device_pp, the
k_solve_wide_pp / k_resume_wide<PP_RESUME> instances) and the tick with Tracking::deceleration
(mpcg_track_device_goal), against the oracle called with each row's own parameters.

The handle is always created with other values in every per-problem field
(test_pparams_host.other_handle_params): a path that reads the handle instead of the row fails
on values.  Tolerances are test_gpu_parity.check_against's: statuses, restoration counts and
iteration counts exact, u0 / traj to 1e-7.
"""
from __future__ import annotations

from decimal import Decimal, getcontext

import numpy as np
import pytest

from test_gpu_parity import check_against, oracle_ref, solver_for, torch_cuda  # noqa: F401
from test_option_matrix import TABLE
from test_pparams_host import decelerate_np, other_handle_params, recipe

pytestmark = pytest.mark.gpu

OUT = ("u0", "traj", "status", "iters", "obj")


def oracle_rows(oracle, dicts, st, cf):
    """The oracle's solve of problem i under dicts[i]: one batch call per distinct parameter set,
    the calls side by side on 16 threads in all."""
    from concurrent.futures import ThreadPoolExecutor

    B = len(dicts)
    N = int(dicts[0]["STEPS"])
    ref = dict(u0=np.zeros((B, 2)), traj=np.zeros((B, 3, N)), obj=np.zeros(B), status=np.zeros(B, np.int32),
               iters=np.zeros(B, np.int32), diag=np.zeros((B, 7), np.int32))
    groups = {}
    for i, d in enumerate(dicts):
        groups.setdefault(tuple(sorted(d.items())), []).append(i)
    per = max(1, 16 // len(groups))
    with ThreadPoolExecutor(min(16, len(groups))) as ex:
        done = list(ex.map(lambda kv: oracle_ref(oracle, dict(kv[0]), st[kv[1]], cf[kv[1]], threads=per), groups.items()))
    for rows, r in zip(groups.values(), done):
        for k in ref:
            ref[k][rows] = r[k]
    return ref


def pp_solver(P, **kw):
    """A handle for the batch of P's horizon and model, every per-problem field another value."""
    return solver_for(other_handle_params(P), **kw)


def is_pp(s, name=None):
    k = s.last_kernel
    assert k.startswith("k_solve_wide_pp<"), k
    assert name is None or k == name, k


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def solve_device_rows(torch, s, st, cf, rows, N):
    """solve_device with pparams; the outputs as numpy arrays by name."""
    B = st.shape[0]
    d = torch.device("cuda:0")
    out = dict(u0=torch.full((B, 2), 7.0, dtype=torch.float64, device=d),
               traj=torch.full((B, 3, N), 7.0, dtype=torch.float64, device=d),
               status=torch.full((B,), -1, dtype=torch.int32, device=d),
               obj=torch.full((B,), 7.0, dtype=torch.float64, device=d),
               iters=torch.full((B,), -1, dtype=torch.int32, device=d),
               diag=torch.full((B, 4), -1, dtype=torch.int32, device=d))
    s.solve_device(dev(torch, st), dev(torch, cf), pparams=dev(torch, rows), **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. heterogeneous rows
@pytest.mark.parametrize("options,kernel", [
    ({}, "k_solve_wide_pp<0,true,double,1,true,2>"),  # (the reference's options: compiled in)
    ({"acceptable_obj_change_tol": 1e30}, "k_solve_wide_pp<0,true,double,1,false,2>"),  # (an inert option: the general one)
])
def test_heterogeneous_rows_benchmark_class(torch_cuda, oracle, infinity_golden, options, kernel):  # noqa: F811
    from conftest import params_from_array
    from mpc_ros_amd import params

    g = infinity_golden
    P = params_from_array(g["params"])
    st, cf = g["state"][:32], g["coeffs"][:32]
    dicts = [recipe(P, i) for i in range(32)]
    ref = oracle_rows(oracle, dicts, st, cf)
    assert (ref["status"] == 1).all() and (ref["diag"][:, 3] == 0).all()
    assert (ref["iters"] != g["iters"][:32]).sum() >= 16  # (the parameters act)
    s = pp_solver(P, **options)
    r = s.solve(st, cf, params_rows=params.rows(dicts))
    is_pp(s, kernel)
    check_against(r, ref)


# ------------------------------------------------------------------ 2. the handle's own rows
def test_rows_equal_to_the_handle_are_the_plain_solve_bitwise(torch_cuda, infinity_golden, features_golden):  # noqa: F811
    from conftest import params_from_array
    from mpc_ros_amd import params

    for g, n in ((infinity_golden, 64), (features_golden["resto_N20"], 4)):
        P = g["P"] if "P" in g else params_from_array(g["params"])
        st, cf = g["state"][:n], g["coeffs"][:n]
        s = solver_for(P)
        plain = s.solve(st, cf)
        assert s.last_kernel.startswith("k_solve_wide<")
        r = s.solve(st, cf, params_rows=params.rows(P, B=n))
        is_pp(s)
        for k in OUT + ("diag",):
            np.testing.assert_array_equal(r[k], plain[k], err_msg=k)


# ------------------------------------------------------------------ 3. across a park and its overflow
PARK_ROWS = {"resto_N20": 4, "resto_N40": 12, "bicycle": 6}


@pytest.mark.parametrize("park_capacity", [0, 1])
@pytest.mark.parametrize("sname", list(PARK_ROWS))
def test_rows_across_a_park(torch_cuda, oracle, features_golden, sname, park_capacity):  # noqa: F811
    """Problems that enter the restoration phase: k_resume_wide<PP_RESUME> rebuilds the row's parameters
    for a parked problem and for the re-solve after a park-area overflow (one park entry).  Even
    rows take the recipe, odd rows the set's own parameters -- not the handle's."""
    from mpc_ros_amd import params

    g = features_golden[sname]
    P, n = g["P"], PARK_ROWS[sname]
    st, cf = g["state"][:n], g["coeffs"][:n]
    dicts = [recipe(P, i) if i % 2 == 0 else dict(P) for i in range(n)]
    ref = oracle_rows(oracle, dicts, st, cf)
    resto = ref["diag"][:, 3] > 0
    assert resto.sum() >= (1 if sname == "bicycle" else 2)
    s = pp_solver(P)
    s.set_park_capacity(park_capacity)
    r = s.solve(st, cf, params_rows=params.rows(dicts))
    is_pp(s)
    check_against(r, ref)
    np.testing.assert_array_equal(r["diag"][:, 2] > 0, resto)
    if park_capacity == 0:
        assert (r["diag"][resto, 2] == 1).all()
    elif resto.sum() >= 2:
        assert (r["diag"][:, 2] == 2).any() and (r["diag"][:, 2] == 1).sum() <= 1


# ------------------------------------------------------------------ 4. instance shapes
SHAPE_KERNEL = {
    "N33": "k_solve_wide_pp<0,false,double,1,false,2>",
    "N40": "k_solve_wide_pp<0,false,double,1,false,2>",
    "N48": "k_solve_wide_pp<0,false,double,1,false,1>",
    "N65": "k_solve_wide_pp<0,false,double,2,false,1>",
    "bicycle_N25": "k_solve_wide_pp<1,true,double,1,false,2>",
    "bicycle_N33": "k_solve_wide_pp<1,false,double,1,false,2>",
    "bicycle_N48": "k_solve_wide_pp<1,false,double,1,false,1>",
    "bicycle_N65": "k_solve_wide_pp<1,false,double,2,false,1>",  # (the eighth instance; not in the table)
}
# (bicycle_N65: the three rows the oracle solves in under 30 iterations -- 0.07 s each at this horizon)
SHAPE_ROWS = {"bicycle_N65": (1, 2, 3)}


@pytest.mark.parametrize("shape", list(SHAPE_KERNEL))
def test_rows_across_instance_shapes(torch_cuda, oracle, infinity_golden, shape):  # noqa: F811
    from mpc_ros_amd import params

    extra = TABLE["shapes"]["params"].get(shape) or dict(TABLE["shapes"]["params"]["bicycle_N48"], STEPS=65)
    P = dict(params.PLUGIN_DEFAULTS, **extra)
    bike = P.get("MODEL", 0) == 1
    rows = list(SHAPE_ROWS.get(shape, range(6)))
    st, cf = infinity_golden["state"][rows], infinity_golden["coeffs"][rows]
    dicts = [recipe(P, i, vary_lf=bike) for i in rows]
    ref = oracle_rows(oracle, dicts, st, cf)
    base = oracle_ref(oracle, P, st, cf)
    assert ((ref["status"] != base["status"]) | (ref["iters"] != base["iters"])
            | (np.abs(ref["u0"] - base["u0"]).max(1) > 1e-9)).any()
    s = pp_solver(P)
    r = s.solve(st, cf, params_rows=params.rows(dicts))
    is_pp(s, SHAPE_KERNEL[shape])
    check_against(r, ref)


# ------------------------------------------------------------------ 5. the ordered launch
def test_rows_follow_the_problem_in_an_ordered_launch(torch_cuda, oracle):  # noqa: F811
    """B = 2,304 > 2,048: the batch runs expected-longest first, so workgroup b solves problem
    order[b] -- with row order[b], not row b."""
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    B = 2304
    st, cf = infinity.make_problems(np.arange(B))
    sets = [recipe(P, i) for i in range(4)]
    dicts = [sets[i % 4] for i in range(B)]
    ref = oracle_rows(oracle, dicts, st, cf)
    s = pp_solver(P)
    r = s.solve(st, cf, params_rows=params.rows(dicts))
    is_pp(s)
    assert s.last_solve_order
    check_against(r, ref)


# ------------------------------------------------------------------ 6. invalid rows
def test_invalid_rows_end_with_status_13_and_nothing_else_changes(torch_cuda, oracle, infinity_golden):  # noqa: F811
    from conftest import params_from_array
    from mpc_ros_amd import params
    from mpc_ros_amd._lib import MpcgError

    torch = torch_cuda
    g = infinity_golden
    P = params_from_array(g["params"])
    N = int(P["STEPS"])
    st, cf = g["state"][:16], g["coeffs"][:16]
    dicts = [recipe(P, i) for i in range(16)]
    rows = params.rows(dicts)
    bad = [3, 7, 11]
    rows[3, params.ROW_KEYS.index("W_A")] = np.nan
    rows[7, params.ROW_KEYS.index("W_V")] = -1.0
    rows[11, params.ROW_KEYS.index("MAXTHR")] = 0.0
    good = [i for i in range(16) if i not in bad]
    ref = oracle_rows(oracle, [dicts[i] for i in good], st[good], cf[good])
    s = pp_solver(P)
    r = solve_device_rows(torch, s, st, cf, rows, N)
    is_pp(s)
    np.testing.assert_array_equal(np.flatnonzero(r["status"] == 13), bad)
    assert (r["iters"][bad] == 0).all() and (r["u0"][bad] == 0).all() and (r["traj"][bad] == 0).all()
    assert np.isnan(r["obj"][bad]).all() and (r["diag"][bad] == 0).all()
    check_against({k: v[good] for k, v in r.items()}, ref)
    # the handle afterwards: a plain solve as a fresh handle's
    Ph = other_handle_params(P)
    after, fresh = s.solve(st, cf), solver_for(Ph).solve(st, cf)
    for k in OUT + ("diag",):
        np.testing.assert_array_equal(after[k], fresh[k], err_msg=k)
    # the host entry point checks the rows first and names the first bad one
    with pytest.raises(MpcgError, match="row 3"):
        s.solve(st, cf, params_rows=rows)


# ------------------------------------------------------------------ 7. graph replay
def test_graph_replay_reads_the_rows_at_replay_time(torch_cuda, infinity_golden):  # noqa: F811
    from conftest import params_from_array
    from mpc_ros_amd import params

    torch = torch_cuda
    g = infinity_golden
    P = params_from_array(g["params"])
    B, N = 64, int(P["STEPS"])
    st, cf = g["state"][:B], g["coeffs"][:B]
    rows_a = params.rows([recipe(P, i) for i in range(B)])
    rows_b = params.rows([recipe(P, 100 + i) for i in range(B)])
    s = pp_solver(P)
    s.reserve(B)
    direct = [solve_device_rows(torch, s, st, cf, rows, N) for rows in (rows_a, rows_b)]
    assert not np.array_equal(direct[0]["u0"], direct[1]["u0"])
    tst, tcf, trows = dev(torch, st), dev(torch, cf), dev(torch, rows_a)
    d = torch.device("cuda:0")
    u0 = torch.empty((B, 2), dtype=torch.float64, device=d)
    status = torch.empty(B, dtype=torch.int32, device=d)
    iters = torch.empty(B, dtype=torch.int32, device=d)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        s.solve_device(tst, tcf, u0, status=status, iters=iters, pparams=trows)  # (warm-up on the capture stream)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        s.solve_device(tst, tcf, u0, status=status, iters=iters, pparams=trows)
    for rows, want in ((rows_a, direct[0]), (rows_b, direct[1])):
        trows.copy_(torch.from_numpy(rows))  # (in place: the captured pointer)
        u0.zero_()
        status.zero_()
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(u0.cpu().numpy(), want["u0"])
        np.testing.assert_array_equal(status.cpu().numpy(), want["status"])
        np.testing.assert_array_equal(iters.cpu().numpy(), want["iters"])


# ------------------------------------------------------------------ 8. the tick with deceleration
def hypot_exact(dx, dy):
    """hypot correctly rounded (the distance the device computes): sqrt of the exact sum of
    squares at 400 digits, rounded once."""
    getcontext().prec = 400
    return np.array([float((Decimal(float(a)) ** 2 + Decimal(float(b)) ** 2).sqrt()) for a, b in zip(dx, dy)])


def test_tick_with_deceleration_matches_oracle_pipeline(torch_cuda, oracle):  # noqa: F811
    torch = torch_cuda
    from mpc_ros_amd import infinity, params
    from mpc_ros_amd.solver import BatchSolver

    P = params.PLUGIN_DEFAULTS
    idx = np.arange(5000, 5000 + 64)
    B = len(idx)
    sc = infinity.draw_scenarios(idx)
    px, py, yaw, plan = infinity.scenario_poses(sc)
    pose = np.stack([px, py, yaw], axis=1)
    vel = np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], axis=1)
    b = np.arange(B)
    f = np.array([0.02, 0.4, 0.9, 1.5])[b % 4]
    dist0 = f * vel[:, 0] ** 2 / P["MAXTHR"]
    goal = np.stack([px + dist0 * np.cos(yaw + 1.0), py + dist0 * np.sin(yaw + 1.0)], axis=1)
    ref_v0 = np.array([0.2, 1.0])[(b // 4) % 2]
    vmax, vmin = 0.7, 0.05
    dist = hypot_exact(pose[:, 0] - goal[:, 0], pose[:, 1] - goal[:, 1])
    want_rv, kind = decelerate_np(dist, vel[:, 0], max(P["MAXTHR"], 0.1), vmax, vmin, ref_v0)
    assert all((kind == k).sum() >= 4 for k in range(4)), np.bincount(kind)
    assert len(set(want_rv.tolist())) >= 8

    s = BatchSolver(0, P)
    cmd = torch.empty((B, 3), dtype=torch.float64, device="cuda:0")
    status = torch.empty(B, dtype=torch.int32, device="cuda:0")
    tpose, tvel, tplan = dev(torch, pose), dev(torch, vel), dev(torch, plan)
    ref_v = dev(torch, ref_v0)
    s.track_device(tpose, tvel, tplan, cmd, status=status, goal=dev(torch, goal), ref_v=ref_v)  # (defaults 0.7, 0.05)
    torch.cuda.synchronize()
    assert s.last_kernel.startswith("k_solve_wide_pp<")
    got_rv = ref_v.cpu().numpy()
    np.testing.assert_array_equal(got_rv, want_rv)
    sts, cfs = [], []
    for i in range(B):
        rc, ost, ocf = oracle.find_best_path(*pose[i], *vel[i], P["DT"], plan[i], True)
        assert rc == 0
        sts.append(ost)
        cfs.append(ocf)
    ref = oracle_rows(oracle, [dict(P, REF_V=float(v)) for v in want_rv], np.array(sts), np.array(cfs))
    assert (ref["status"] == 1).all()
    thr = ref["u0"][:, 1]
    speed = np.minimum(vel[:, 0] + thr * P["DT"], want_rv)
    c = cmd.cpu().numpy()
    np.testing.assert_array_equal(status.cpu().numpy(), ref["status"])
    np.testing.assert_allclose(c[:, 1], ref["u0"][:, 0], atol=1e-7)
    np.testing.assert_allclose(c[:, 2], thr, atol=1e-7)
    np.testing.assert_allclose(c[:, 0], speed, atol=1e-7)
    # the next tick, far from the goal: REF_V persists
    far = goal + 10.0
    s.track_device(tpose, tvel, tplan, cmd, status=status, goal=dev(torch, far), ref_v=ref_v)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ref_v.cpu().numpy(), want_rv)
    c2 = cmd.cpu().numpy()
    np.testing.assert_array_equal(c2, c)  # (the same REF_V, the same solve)


@pytest.mark.parametrize("M", [11, 65])
def test_plain_tick_is_the_goal_tick_far_from_every_goal(torch_cuda, M):  # noqa: F811
    """64 robots of the benchmark generator, plans of 11 waypoints and of 65 (the shortest that
    takes the HBM-workspace QR): mpcg_track_device equals mpcg_track_device_goal with every goal
    10 m away in x and y and the handle's REF_V in ref_v -- cmd, traj and status bitwise, ref_v
    unchanged.  The two run different solver instances (k_solve_wide, k_solve_wide_pp) on one
    pipeline."""
    torch = torch_cuda
    from mpc_ros_amd import params
    from mpc_ros_amd.solver import BatchSolver

    P = params.PLUGIN_DEFAULTS
    B, N = 64, int(P["STEPS"])
    s = BatchSolver(0, P)
    pose, vel, plan = s.synth_infinity_device(9000, B, M=M)
    out = []
    for goal in (False, True):
        cmd = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0")
        traj = torch.full((B, 3, N), 7.0, dtype=torch.float64, device="cuda:0")
        status = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
        ref_v = torch.full((B,), float(P["REF_V"]), dtype=torch.float64, device="cuda:0")
        kw = dict(goal=(pose[:, :2] + 10.0).contiguous(), ref_v=ref_v) if goal else {}
        s.track_device(pose, vel, plan, cmd, traj=traj, status=status, **kw)
        torch.cuda.synchronize()
        assert s.last_kernel.startswith("k_solve_wide_pp<" if goal else "k_solve_wide<"), s.last_kernel
        out.append((cmd.cpu().numpy(), traj.cpu().numpy(), status.cpu().numpy()))
        assert (ref_v.cpu().numpy() == P["REF_V"]).all()
    for name, a, b in zip(("cmd", "traj", "status"), *out):
        assert a.tobytes() == b.tobytes(), name
    assert (out[0][0] != 7.0).all() and (out[0][2] != -7).all()  # (written, not the fill values)


def test_tick_argument_errors_leave_ref_v_alone(torch_cuda):  # noqa: F811
    """A plan of fewer than 4 waypoints is refused before anything is queued: ref_v (in/out) is
    not rewritten by a call that fails."""
    torch = torch_cuda
    from mpc_ros_amd import params
    from mpc_ros_amd._lib import MpcgError
    from mpc_ros_amd.solver import BatchSolver

    s = BatchSolver(0, params.PLUGIN_DEFAULTS)
    B = 8
    pose = dev(torch, np.zeros((B, 3)))
    vel = dev(torch, np.full((B, 3), 0.5))
    ref_v = dev(torch, np.full(B, 1.0))
    cmd = torch.empty((B, 3), dtype=torch.float64, device="cuda:0")
    with pytest.raises(MpcgError, match="M "):
        s.track_device(pose, vel, dev(torch, np.zeros((B, 3, 2))), cmd, goal=dev(torch, np.zeros((B, 2))), ref_v=ref_v)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ref_v.cpu().numpy(), np.full(B, 1.0))  # (at the goal the rule would give 0.05)


# ------------------------------------------------------------------ 9. fp32
def test_fp32_with_rows_is_refused(torch_cuda, infinity_golden):  # noqa: F811
    from mpc_ros_amd import params
    from mpc_ros_amd._lib import MpcgError

    torch = torch_cuda
    P = params.PLUGIN_DEFAULTS
    st, cf = infinity_golden["state"][:4], infinity_golden["coeffs"][:4]
    rows = params.rows(P, B=4)
    s = solver_for(P, dtype="fp32")
    with pytest.raises(MpcgError, match="fp32"):
        s.solve(st, cf, params_rows=rows)
    with pytest.raises(MpcgError, match="fp32"):
        s.solve_device(dev(torch, st), dev(torch, cf), torch.empty((4, 2), dtype=torch.float64, device="cuda:0"),
                       pparams=dev(torch, rows))
    with pytest.raises(MpcgError, match="fp32"):
        s.track_device(dev(torch, np.zeros((4, 3))), dev(torch, np.zeros((4, 3))), dev(torch, np.zeros((4, 11, 2))),
                       torch.empty((4, 3), dtype=torch.float64, device="cuda:0"),
                       goal=dev(torch, np.zeros((4, 2))), ref_v=dev(torch, np.ones(4)))
    assert s.solve(st, cf)["status"].tolist() == infinity_golden["status"][:4].tolist()
