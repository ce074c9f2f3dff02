"""GPU: the caller side of MPC::Solve on the device -- Tracking::findBestPath's
preprocessing (mpcg_preprocess_device) and the whole control tick (mpcg_track_device:
preprocessing, solve, post-processing of driving_state.cpp:262-269).

References: the oracle's restatement (oracle/preprocess.c) and its committed fixtures
(tests/golden/preprocess.npz), the vectorised NumPy version used to build the
benchmark inputs (mpc_ros_amd/infinity.py), and the oracle's solve.  Tolerance: the
Householder QR runs in the oracle's operation order (differences are FMA contraction
only), 1e-11 on state/coeffs; the tick's commands at the solve's 1e-7.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import load_npz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


def _solver(P=None):
    from mpc_ros_amd import params
    from mpc_ros_amd.solver import BatchSolver

    return BatchSolver(0, P or params.PLUGIN_DEFAULTS)


def _run_preprocess(torch, s, pose, vel, plan, delay=True):
    dev = torch.device("cuda:0")
    B = pose.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    st = torch.empty((B, 6), dtype=torch.float64, device=dev)
    cf = torch.empty((B, 4), dtype=torch.float64, device=dev)
    s.preprocess_device(t(pose), t(vel), t(plan), st, cf, delay_mode=delay)
    torch.cuda.synchronize()
    return st.cpu().numpy(), cf.cpu().numpy()


def test_preprocess_matches_oracle_fixtures(torch_cuda):
    g = load_npz("preprocess.npz")
    from mpc_ros_amd import params

    s = _solver(dict(params.PLUGIN_DEFAULTS, DT=float(g["dt"])))
    st, cf = _run_preprocess(torch_cuda, s, g["pose"], g["vel"], g["plan"])
    np.testing.assert_allclose(cf, g["coeffs"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(st, g["state"], rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("delay", [True, False])
def test_preprocess_matches_benchmark_generator(torch_cuda, delay):
    from mpc_ros_amd import infinity

    idx = np.arange(1000, 1000 + 4096)
    sc = infinity.draw_scenarios(idx)
    px, py, yaw, plan = infinity.scenario_poses(sc)
    ref_st, ref_cf = infinity.find_best_path(px, py, yaw, sc["v"], sc["w_prev"], sc["a_prev"], 0.1, plan, delay)
    pose = np.stack([px, py, yaw], axis=1)
    vel = np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], axis=1)
    st, cf = _run_preprocess(torch_cuda, _solver(), pose, vel, plan, delay)
    np.testing.assert_allclose(cf, ref_cf, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(st, ref_st, rtol=1e-9, atol=1e-10)


def test_preprocess_rejects_short_plans(torch_cuda):
    """polyfit asserts order 3 <= M - 1 (driving_state.cpp:286): M < 4 is an API error."""
    from mpc_ros_amd._lib import MpcgError

    pose = np.zeros((2, 3))
    with pytest.raises(MpcgError):
        _run_preprocess(torch_cuda, _solver(), pose, pose, np.zeros((2, 3, 2)))


@pytest.mark.parametrize("M", [4, 11, 17, 40, 64, 65, 100, 257])
def test_preprocess_plan_lengths(torch_cuda, oracle, M):
    """Short, medium and long plans (M > 16 takes the 64-row kernel, M > 64 the kernel with
    its QR in an HBM workspace: findBestPath takes any plan length) against the oracle."""
    rng = np.random.default_rng(M)
    B = 96
    pose = np.stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
    vel = np.stack([rng.uniform(0, 0.8, B), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)], axis=1)
    s = np.linspace(0.0, 5.0, M)
    plan = np.empty((B, M, 2))
    for b in range(B):
        h0, k0 = rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4)
        hd = h0 + k0 * s
        plan[b, :, 0] = pose[b, 0] + rng.uniform(-0.3, 0.3) + np.cumsum(np.cos(hd)) * (s[1] - s[0] if M > 1 else 0)
        plan[b, :, 1] = pose[b, 1] + rng.uniform(-0.3, 0.3) + np.cumsum(np.sin(hd)) * (s[1] - s[0] if M > 1 else 0)
    st, cf = _run_preprocess(torch_cuda, _solver(), pose, vel, plan)
    for b in range(B):
        rc, ost, ocf = oracle.find_best_path(*pose[b], *vel[b], 0.1, plan[b], True)
        assert rc == 0
        np.testing.assert_allclose(cf[b], ocf, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st[b], ost, rtol=1e-9, atol=1e-9)


def test_track_tick_matches_oracle_pipeline(torch_cuda, oracle):
    """cmd = (speed, w, throttle) of one control tick against oracle preprocessing +
    oracle solve + driving_state.cpp:262-269."""
    torch = torch_cuda
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    idx = np.arange(5000, 5000 + 64)
    sc = infinity.draw_scenarios(idx)
    px, py, yaw, plan = infinity.scenario_poses(sc)
    pose = np.stack([px, py, yaw], axis=1)
    vel = np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], axis=1)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    B = len(idx)
    cmd = torch.empty((B, 3), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _solver(P).track_device(t(pose), t(vel), t(plan), cmd, status=status)
    torch.cuda.synchronize()
    cmd = cmd.cpu().numpy()
    sts, cfs = [], []
    for b in range(B):
        rc, ost, ocf = oracle.find_best_path(*pose[b], *vel[b], P["DT"], plan[b], True)
        assert rc == 0
        sts.append(ost)
        cfs.append(ocf)
    ref = oracle.mpc_solve_batch(P, np.array(sts), np.array(cfs), opts=oracle.ref_opts(int(P["STEPS"])), nthreads=16)
    w = ref["u0"][:, 0]
    thr = ref["u0"][:, 1]
    speed = np.minimum(vel[:, 0] + thr * P["DT"], P["REF_V"])
    np.testing.assert_allclose(cmd[:, 1], w, atol=1e-7)
    np.testing.assert_allclose(cmd[:, 2], thr, atol=1e-7)
    np.testing.assert_allclose(cmd[:, 0], speed, atol=1e-7)
    np.testing.assert_array_equal(status.cpu().numpy(), ref["status"])


def test_track_tick_equals_solve_on_preprocessed_inputs(torch_cuda):
    """At the benchmark size: the fused tick's controls equal a solve of the
    separately preprocessed problems (same kernels, same inputs)."""
    torch = torch_cuda
    from mpc_ros_amd import infinity

    B = 65536
    sc = infinity.draw_scenarios(np.arange(B))
    px, py, yaw, plan = infinity.scenario_poses(sc)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    pose, vel, tplan = t(np.stack([px, py, yaw], 1)), t(np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], 1)), t(plan)
    s = _solver()
    cmd = torch.empty((B, 3), dtype=torch.float64, device=dev)
    s.track_device(pose, vel, tplan, cmd)
    st = torch.empty((B, 6), dtype=torch.float64, device=dev)
    cf = torch.empty((B, 4), dtype=torch.float64, device=dev)
    s.preprocess_device(pose, vel, tplan, st, cf)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    s.solve_device(st, cf, u0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cmd[:, 1:].cpu().numpy(), u0.cpu().numpy())


def test_track_tick_long_plans_match_oracle(torch_cuda, oracle):
    """A whole control tick with plans of 120 waypoints (the preprocessing's HBM-workspace
    QR): commands against the oracle pipeline."""
    torch = torch_cuda
    from mpc_ros_amd import params

    P = params.PLUGIN_DEFAULTS
    rng = np.random.default_rng(120)
    B, M = 48, 120
    pose = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-np.pi, np.pi, B)], axis=1)
    vel = np.stack([rng.uniform(0.2, 0.8, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    s = np.linspace(0.0, 3.0, M)
    plan = np.empty((B, M, 2))
    for b in range(B):
        hd = pose[b, 2] + rng.uniform(-0.2, 0.2) + rng.uniform(-0.3, 0.3) * s
        plan[b, :, 0] = pose[b, 0] + np.cumsum(np.cos(hd)) * (s[1] - s[0])
        plan[b, :, 1] = pose[b, 1] + np.cumsum(np.sin(hd)) * (s[1] - s[0])
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    cmd = torch.empty((B, 3), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _solver(P).track_device(t(pose), t(vel), t(plan), cmd, status=status)
    torch.cuda.synchronize()
    cmd = cmd.cpu().numpy()
    sts, cfs = [], []
    for b in range(B):
        rc, ost, ocf = oracle.find_best_path(*pose[b], *vel[b], P["DT"], plan[b], True)
        assert rc == 0
        sts.append(ost)
        cfs.append(ocf)
    ref = oracle.mpc_solve_batch(P, np.array(sts), np.array(cfs), opts=oracle.ref_opts(int(P["STEPS"])), nthreads=16)
    np.testing.assert_array_equal(status.cpu().numpy(), ref["status"])
    np.testing.assert_allclose(cmd[:, 1], ref["u0"][:, 0], atol=1e-7)
    np.testing.assert_allclose(cmd[:, 2], ref["u0"][:, 1], atol=1e-7)


def test_two_streams_share_one_handle(torch_cuda):
    """One handle, two streams, batches above the solve-order threshold (its sort scratch,
    spill areas and track buffers are the handle's): the second solve is queued without a
    host sync and waits on the first one's scratch use; both equal their solo results."""
    torch = torch_cuda
    from mpc_ros_amd import infinity

    B = 8192
    dev = torch.device("cuda:0")
    s = _solver()
    ins = []
    for off in (0, 100000):
        st, cf = infinity.make_problems(np.arange(off, off + B))
        ins.append((torch.from_numpy(st).to(dev), torch.from_numpy(cf).to(dev)))
    solo = []
    for st, cf in ins:
        u = torch.empty((B, 2), dtype=torch.float64, device=dev)
        s.solve_device(st, cf, u)
        torch.cuda.synchronize()
        solo.append(u.cpu().numpy())
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = [torch.empty((B, 2), dtype=torch.float64, device=dev) for _ in ins]
    s.solve_device(ins[0][0], ins[0][1], outs[0], stream=s1)
    s.solve_device(ins[1][0], ins[1][1], outs[1], stream=s2)
    torch.cuda.synchronize()
    for o, r in zip(outs, solo):
        np.testing.assert_array_equal(o.cpu().numpy(), r)


def test_two_kinds_of_tick_on_two_streams_share_the_scratch(torch_cuda):
    """One handle: a plain tick of 96 robots on one stream and a K = 2 rollout of the 96-robot
    scene on another, queued back to back without a host synchronisation (either first).  Both
    use the handle's one tick scratch, from the same offsets; the second waits for the first
    one's use, and each equals its solo result bitwise.  (Each runs alone first: the buffers
    have grown.)"""
    torch = torch_cuda
    from mpc_ros_amd import infinity
    from test_gpu_rollout import Loop

    loop = Loop(torch)
    s, B, N = loop.s, loop.B, loop.s.N
    dev = torch.device("cuda:0")
    sc = infinity.draw_scenarios(np.arange(7000, 7000 + B))
    px, py, yaw, plan = infinity.scenario_poses(sc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    pose, vel, tplan = t(np.stack([px, py, yaw], 1)), t(np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], 1)), t(plan)

    def outputs():
        """fresh outputs of both, the rollout's inputs restored; nothing pending on the device"""
        loop.restore()
        tick = dict(cmd=torch.full((B, 3), 7.0, dtype=torch.float64, device=dev),
                    traj=torch.full((B, 3, N), 7.0, dtype=torch.float64, device=dev),
                    status=torch.full((B,), -7, dtype=torch.int32, device=dev))
        logs = s.rollout_logs(2, B)
        torch.cuda.synchronize()
        return tick, logs

    def plain(tick, stream=None):
        s.track_device(pose, vel, tplan, tick["cmd"], traj=tick["traj"], status=tick["status"], stream=stream)

    def results(tick, logs):
        torch.cuda.synchronize()
        r = {"tick." + k: v.cpu().numpy() for k, v in tick.items()}
        r.update({"log." + k: v.cpu().numpy() for k, v in logs.items()})
        r.update({"final." + k: v for k, v in loop.final().items()})
        return r

    tick, logs = outputs()
    plain(tick)
    torch.cuda.synchronize()
    loop.call(2, logs)
    solo = results(tick, logs)
    assert (solo["tick.cmd"] != 7.0).all() and (solo["log.iters"][0] > 0).sum() > 80
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for plain_first in (True, False):
        tick, logs = outputs()
        if plain_first:
            plain(tick, stream=s1)
        loop.call(2, logs, stream=s2)
        if not plain_first:
            plain(tick, stream=s1)
        both = results(tick, logs)
        for name in solo:
            assert both[name].tobytes() == solo[name].tobytes(), (name, plain_first)


def test_synthetic_robots_on_device_match_host_generator(torch_cuda):
    """mpcg_synth_infinity_device: the benchmark's robots generated on the GPU from (seed, global
    index) equal infinity.py's host generator (the integer hash bitwise, the trigonometry within
    rounding), for a slice that does not start at 0 (a rank's shard); through the device
    preprocessing they give MPC::Solve's inputs of infinity.make_problems."""
    torch = torch_cuda
    from mpc_ros_amd import infinity, params

    P = params.PLUGIN_DEFAULTS
    s = _solver(P)
    start, B = 3 * 65536 + 17, 4096
    pose, vel, plan = s.synth_infinity_device(start, B)
    torch.cuda.synchronize()
    idx = np.arange(start, start + B)
    sc = infinity.draw_scenarios(idx)
    px, py, yaw, hplan = infinity.scenario_poses(sc)
    np.testing.assert_allclose(pose.cpu().numpy(), np.stack([px, py, yaw], 1), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(vel.cpu().numpy(), np.stack([sc["v"], sc["w_prev"], sc["a_prev"]], 1))
    np.testing.assert_allclose(plan.cpu().numpy(), hplan, rtol=0, atol=1e-12)
    st = torch.empty((B, 6), dtype=torch.float64, device=pose.device)
    cf = torch.empty((B, 4), dtype=torch.float64, device=pose.device)
    s.preprocess_device(pose, vel, plan, st, cf)
    torch.cuda.synchronize()
    hst, hcf = infinity.make_problems(idx)
    np.testing.assert_allclose(st.cpu().numpy(), hst, rtol=0, atol=1e-9)
    np.testing.assert_allclose(cf.cpu().numpy(), hcf, rtol=1e-9, atol=1e-9)
