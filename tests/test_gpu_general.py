"""GPU parity away from the infinity course: the solver on general states and polynomials
(tests/golden/general.npz), the preprocessing and the tick on straight and circular plans that take
the branches of findBestPath's heading rule (tests/off_course.py).

Every other solver test draws its problems from mpc_ros_amd/infinity.py: y = 0, x = v dt in
[0, 0.08], the cubic fit of one curve seen from nearby.  The general set has any pose (y != 0, the
polynomial at x < 0 and |x| > 2), speeds from reversing to above REF_V, far-off errors with steep
polynomials, exact lines and the all-zero problem.  Every fixture row is pinned by the oracle under
three variants of its linear algebra (tests/golden/make_goldens.py general) and reproduced by the
host emulation of the kernel's code (tests/test_core_host.py), so a mismatch here is device against
emulation on a known row.

The records, the certificate and the sensitivities of general_N20 and general_bicycle_N25 on the
device are cases of tests/test_gpu_solution.py, tests/test_gpu_kkt.py and tests/test_gpu_sens.py's own
shape tables.  Tolerances are those modules' and tests/test_gpu_parity.py's; nothing here has a
bound of its own.
"""
from __future__ import annotations

import numpy as np
import pytest

import off_course
from test_gpu_headline import HEADLINE, LONE
from test_gpu_parity import ATOL, check_against, solver_for, torch_cuda  # noqa: F401
from test_solution_host import GENERAL_SHAPES, fixture_set

pytestmark = pytest.mark.gpu

# the instance class of each shape (wide_plan.h wide_class): split sweeps for N <= 32, stage blocks
SHAPE_CLASS = {"N20": ("true", "1"), "N40": ("false", "1"), "N65": ("false", "2"), "bicycle_N25": ("true", "1"),
               "class_defaults": ("true", "1"), "N3": ("true", "1")}
OUT = ("u0", "traj", "status", "iters", "obj", "diag")


@pytest.mark.parametrize("shape", GENERAL_SHAPES)
def test_general_rows_match_oracle(torch_cuda, shape):  # noqa: F811
    """Every row of a shape: status, restoration count, u0 and trajectory at 1e-7, iterations exact."""
    P, g = fixture_set("general_" + shape)
    assert set(g["category"]) == {"pose", "speed", "far", "line"}
    s = solver_for(P)
    r = s.solve(np.ascontiguousarray(g["state"]), np.ascontiguousarray(g["coeffs"]))
    k = s.last_kernel[:-1].split(",")
    assert (k[1], k[3]) == SHAPE_CLASS[shape], s.last_kernel
    if shape == "N20":
        assert s.last_kernel == LONE
    du, dt = np.abs(r["u0"] - g["u0"]).max(), np.abs(r["traj"] - g["traj"]).max()
    print(f"general_{shape}: {len(g['status'])} rows, max |u0 - oracle| {du:.3e}, trajectory {dt:.3e}, "
          f"iterations equal on {np.mean(r['iters'] == g['iters']):.3f}")
    check_against(r, g, min_same_iters=1.0)


def tiled(torch, name, B, kernel):
    """A set's rows tiled to a batch of B (no oracle call): the instance that ran, every copy
    against its fixture row, and the copies of a row byte-equal to each other."""
    P, g = fixture_set(name)
    n = len(g["status"])
    idx = np.arange(B) % n
    s = solver_for(P)
    r = s.solve(np.ascontiguousarray(g["state"][idx]), np.ascontiguousarray(g["coeffs"][idx]))
    assert s.last_kernel == kernel and s.last_solve_order
    check_against(r, {k: g[k][idx] for k in OUT if k in g}, min_same_iters=1.0)
    for k in OUT:
        np.testing.assert_array_equal(r[k], r[k][:n][idx], err_msg=k)


def test_general_rows_through_the_benchmarks_instance(torch_cuda):  # noqa: F811
    """4,097 problems, the smallest batch the benchmark's own instance takes (wide_plan.h kLoneBatch),
    in its expected-longest-first solve order."""
    tiled(torch_cuda, "general_N20", 4097, HEADLINE)


def test_general_rows_through_the_bicycle_instance_in_an_ordered_batch(torch_cuda):  # noqa: F811
    """The bicycle's instance (the same at every batch size) at 2,049 problems, the smallest batch
    that is solved in expected-longest-first order (wide_plan.h kOrderMinBatch)."""
    tiled(torch_cuda, "general_bicycle_N25", 2049, "k_solve_wide<1,true,double,1,true,2>")


def test_general_pose_rows_sensitivities_against_the_dense_solve(torch_cuda, oracle):  # noqa: F811
    """The device's gains and dx of 8 `pose` rows (y != 0, any heading) against the dense numpy solve
    of the definition's system on the device's own records."""
    from test_gpu_sens import solved
    from test_sens_host import SENS_DENSE_BOUND, dense_reference, rel_err

    r = solved(torch_cuda, "general_N20")
    _, g = fixture_set("general_N20")
    rows = np.flatnonzero(g["category"] == "pose")[:8]
    N = r["N"]
    assert len(rows) == 8 and (r["status"][rows] == 1).all() and (r["info"][rows] == 0).all()
    assert (np.abs(r["state"][rows, 1]) > 0).all()
    ref = [dense_reference(oracle, r["P"], r["coeffs"][b], r["sol"][b]) for b in rows]
    assert all(i == (8 * N - 2, 6 * N) for _, _, i in ref)
    e = rel_err(r["gain"][rows], r["dx"][rows], np.array([g_ for g_, _, _ in ref]), np.array([d for _, d, _ in ref]))
    print(f"general_N20 pose rows {rows.tolist()}: device against dense max |delta| / max(1, max|G|) = {e.max():.3e} "
          f"(bound {SENS_DENSE_BOUND:.1e})")
    assert (e <= SENS_DENSE_BOUND).all()


# ---------------------------------------------------------------- preprocessing and the tick
def dev(torch, a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def preprocess(torch, s, pose, vel, plan, delay, count=None):
    B = len(pose)
    st = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda:0")
    cf = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda:0")
    s.preprocess_device(dev(torch, pose), dev(torch, vel), dev(torch, plan), st, cf, delay_mode=delay,
                        count=None if count is None else dev(torch, count, np.int32))
    torch.cuda.synchronize()
    return st.cpu().numpy(), cf.cpu().numpy()


def oracle_preprocess(oracle, pose, vel, plan, delay, counts=None):
    ref = [oracle.find_best_path(*pose[b], *vel[b], 0.1, plan[b] if counts is None else plan[b, :counts[b]], delay)
           for b in range(len(pose))]
    assert all(rc == 0 for rc, _, _ in ref)
    return np.array([s for _, s, _ in ref]), np.array([c for _, _, c in ref])


@pytest.mark.parametrize("M", off_course.PLAN_LENGTHS)
def test_preprocess_off_course_plans(torch_cuda, oracle, M):  # noqa: F811
    """Axis-aligned plans (gy == 0, gx == 0), the +2 pi wrap, the 1.8 pi cut-off, a path behind the
    robot, one 5 m beside it, one it faces backwards along, a circle of 0.5 m radius; at plan lengths
    without a sampled increment (4, 5, 6), with one (7), at the benchmark's 11, in the 64-row kernel
    (40) and the HBM-workspace kernel (70); with and without delay mode.  Every robot against the
    oracle, relative 1e-9 (the circle's cubic through 4 points has large coefficients); on the
    oracle's output every robot takes the branch its plan is named for."""
    from mpc_ros_amd import params

    pose, vel, plan, names = off_course.robots(M)
    s = solver_for(dict(params.PLUGIN_DEFAULTS))
    for delay in (True, False):
        ost, ocf = oracle_preprocess(oracle, pose, vel, plan, delay)
        if not delay:
            seen = off_course.assert_branches(M, pose, plan, names, ost)
            want = {"no_increment"} if M <= 6 else {"gx_zero", "gy_zero", "wrap", "cutoff", "backwards"}
            assert seen == want | {"behind", "beside"}
        st, cf = preprocess(torch_cuda, s, pose, vel, plan, delay)
        print(f"M = {M}, delay {delay}: max |c| {np.abs(ocf).max():.3e}, coeffs max |delta| {np.abs(cf - ocf).max():.3e}, "
              f"state max |delta| {np.abs(st - ost).max():.3e}")
        np.testing.assert_allclose(cf, ocf, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st, ost, rtol=1e-9, atol=1e-9)
        if not delay:  # the branches that give etheta = 0 give it exactly
            np.testing.assert_array_equal(st[:, 5] == 0.0, ost[:, 5] == 0.0)


def test_preprocess_off_course_plans_with_a_count_per_robot(torch_cuda, oracle):  # noqa: F811
    """The same plans in rows of 11 waypoints with the counts 4..11 mixed inside each wavefront, so
    k_find_best_path_n makes eight passes per wavefront: each robot against the oracle on its own
    count (rows past the count hold NaN: they are not read)."""
    from mpc_ros_amd import params

    pose, vel, plan, names = off_course.robots(11)
    B = len(pose)
    # (8 plans, 9 velocity triples, 8 counts: robot b's count steps with b and with b // 8, so every
    # plan meets every count)
    counts = (4 + (np.arange(B) + np.arange(B) // 8) % 8).astype(np.int32)
    assert set(counts[:64]) == set(range(4, 12)) and len({(names[b], counts[b]) for b in range(B)}) == 64
    for b in range(B):
        plan[b, counts[b]:] = np.nan
    s = solver_for(dict(params.PLUGIN_DEFAULTS))
    for delay in (True, False):
        ost, ocf = oracle_preprocess(oracle, pose, vel, plan, delay, counts)
        st, cf = preprocess(torch_cuda, s, pose, vel, plan, delay, count=counts)
        for b in range(B):
            np.testing.assert_allclose(cf[b], ocf[b], rtol=1e-9, atol=1e-9, err_msg=f"{b} {names[b]} {counts[b]}")
            np.testing.assert_allclose(st[b], ost[b], rtol=1e-9, atol=1e-9, err_msg=f"{b} {names[b]} {counts[b]}")
        if not delay:
            # counts 4..6 sample no increment, 7..11 one to two: the heading rule on the robot's own count
            assert (ost[counts <= 6, 5] == 0.0).all() and (ost[counts >= 7, 5] != 0.0).any()
            np.testing.assert_array_equal(st[:, 5] == 0.0, ost[:, 5] == 0.0)


def test_track_tick_off_course_matches_oracle_pipeline(torch_cuda, oracle):  # noqa: F811
    """One whole tick over the 72 robots at M = 11 against oracle preprocessing + oracle solve +
    driving_state.cpp:262-269: status exact, commands at 1e-7.  (On these 72 states the oracle's
    status and iteration count are the same with its dense solve, its structured solve and one
    refinement step -- checked when the test was written: no robot is left out.)"""
    torch = torch_cuda
    from mpc_ros_amd import params

    P = dict(params.PLUGIN_DEFAULTS)
    pose, vel, plan, names = off_course.robots(11)
    B, N = len(pose), int(P["STEPS"])
    cmd = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda:0")
    traj = torch.full((B, 3, N), 7.0, dtype=torch.float64, device="cuda:0")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    solver_for(P).track_device(dev(torch, pose), dev(torch, vel), dev(torch, plan), cmd, traj=traj, status=status)
    torch.cuda.synchronize()
    cmd = cmd.cpu().numpy()
    ost, ocf = oracle_preprocess(oracle, pose, vel, plan, True)
    ref = oracle.mpc_solve_batch(P, ost, ocf, opts=oracle.ref_opts(N), nthreads=16)
    np.testing.assert_array_equal(status.cpu().numpy(), ref["status"])
    assert (ref["status"] == 1).all()
    w, thr = ref["u0"][:, 0], ref["u0"][:, 1]
    print(f"tick: max |w - oracle| {np.abs(cmd[:, 1] - w).max():.3e}, throttle {np.abs(cmd[:, 2] - thr).max():.3e}")
    np.testing.assert_allclose(cmd[:, 1], w, rtol=0, atol=ATOL)
    np.testing.assert_allclose(cmd[:, 2], thr, rtol=0, atol=ATOL)
    np.testing.assert_allclose(cmd[:, 0], np.minimum(vel[:, 0] + thr * P["DT"], P["REF_V"]), rtol=0, atol=ATOL)
    np.testing.assert_allclose(traj.cpu().numpy(), ref["traj"], rtol=0, atol=ATOL)
