"""Host-side logic of the product package (no GPU): parameter semantics of the
reference's MPC / LoadParams, the synthetic problem generator, sharding."""
from __future__ import annotations

import os

import numpy as np
import pytest

from mpc_ros_amd import dist, infinity, params
from mpc_ros_amd.mpc import MPC


def test_mpc_defaults_match_reference_constructor():
    m = MPC()
    p = m.effective_params()
    # MPC::MPC() mpc_planner.cpp:226-230 and FG_eval ctor :47-57
    assert p["STEPS"] == 20 and p["ANGVEL"] == 3.0 and p["MAXTHR"] == 1.0 and p["BOUND"] == 1e3
    assert p["DT"] == 0.1 and p["REF_V"] == 0.5 and p["W_CTE"] == 100 and p["W_V"] == 1 and p["W_DA"] == 0


def test_load_params_semantics():
    m = MPC()
    m.LoadParams(dict(params.PLUGIN_DEFAULTS, STEPS=25.9))
    p = m.effective_params()
    assert p["STEPS"] == 25  # double -> int truncation (mpc_planner.cpp:247)
    assert p["W_CTE"] == 1000 and p["ANGVEL"] == 1.0
    # a later map without some keys: MPC-level keys keep their value, FG keys revert
    m.LoadParams({"W_V": 7.0})
    p = m.effective_params()
    assert p["STEPS"] == 25 and p["ANGVEL"] == 1.0 and p["BOUND"] == 1000
    assert p["W_V"] == 7.0 and p["W_CTE"] == 100.0 and p["REF_V"] == 0.5


def test_generator_is_shard_independent():
    a_st, a_cf = infinity.make_problems(np.arange(0, 300))
    b_st, b_cf = infinity.make_problems(np.arange(137, 300))
    np.testing.assert_array_equal(a_st[137:], b_st)
    np.testing.assert_array_equal(a_cf[137:], b_cf)


def test_generator_ranges():
    sc = infinity.draw_scenarios(np.arange(20000))
    assert sc["lateral"].min() >= -0.45 and sc["lateral"].max() <= 0.30
    assert sc["heading_err"].min() >= -0.85 and sc["heading_err"].max() <= 1.10
    assert sc["v"].min() >= 0 and sc["v"].max() <= 0.8
    st, cf = infinity.make_problems(np.arange(4096))
    assert np.isfinite(st).all() and np.isfinite(cf).all()
    # delay-mode prediction (driving_state.cpp:242-256): y_act = 0, x_act = v dt >= 0
    assert (st[:, 1] == 0).all() and (st[:, 0] >= 0).all()


def test_generator_matches_golden_preprocess():
    from conftest import load_npz

    z = load_npz("preprocess.npz")
    st, cf = infinity.find_best_path(z["pose"][:, 0], z["pose"][:, 1], z["pose"][:, 2], z["vel"][:, 0],
                                     z["vel"][:, 1], z["vel"][:, 2], float(z["dt"]), z["plan"])
    np.testing.assert_allclose(st, z["state"], atol=1e-11)
    np.testing.assert_allclose(cf, z["coeffs"], atol=1e-9, rtol=1e-9)


@pytest.mark.parametrize("M", [4, 5, 6, 7, 11, 40, 70])
def test_off_course_plans_take_their_branches(oracle, M):
    """tests/off_course.py's robots (the inputs of tests/test_gpu_general.py's preprocessing and
    tick tests): on the oracle's output every plan takes the branch of the heading rule it is named
    for, and the vectorised NumPy preprocessing agrees with the oracle on them, with and without
    delay mode."""
    import off_course

    assert M in off_course.PLAN_LENGTHS
    pose, vel, plan, names = off_course.robots(M)
    seen = set()
    for delay in (True, False):
        ref = [oracle.find_best_path(*pose[b], *vel[b], 0.1, plan[b], delay) for b in range(len(pose))]
        assert all(rc == 0 for rc, _, _ in ref)
        ost, ocf = np.array([s for _, s, _ in ref]), np.array([c for _, _, c in ref])
        st, cf = infinity.find_best_path(pose[:, 0], pose[:, 1], pose[:, 2], vel[:, 0], vel[:, 1], vel[:, 2], 0.1, plan,
                                         delay)
        np.testing.assert_allclose(cf, ocf, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st, ost, rtol=1e-9, atol=1e-9)
        if not delay:
            seen = off_course.assert_branches(M, pose, plan, names, ost)
    want = {"no_increment"} if M <= 6 else {"gx_zero", "gy_zero", "wrap", "cutoff", "backwards"}
    assert seen == want | {"behind", "beside"}


@pytest.mark.parametrize("total,world", [(10, 3), (524288, 8), (5, 8), (64, 1)])
def test_shard_covers_exactly(total, world):
    seen = []
    for r in range(world):
        s, c = dist.shard(total, r, world)
        seen.extend(range(s, s + c))
        assert c <= dist.max_shard(total, world)
    assert seen == list(range(total))


def test_build_reads_kernel_resource_remarks():
    """build.kernel_resources parses hipcc's kernel-resource-usage remarks; the build
    refuses a solve kernel whose LDS is not all dynamic (static LDS would overlap the
    solver's layout, which starts at address 0)."""
    from mpc_ros_amd import build

    text = "\n".join([
        "x.hip:39:1: remark: Function Name: _ZN4mpcg12k_solve_wideILi0ELb1EdLi1ELb1EEEvNS_8WideArgsE [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:39:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:39:1: remark:     ScratchSize [bytes/lane]: 128 [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:39:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:39:1: remark:     SGPRs Spill: 341 [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:39:1: remark:     LDS Size [bytes/block]: 4096 [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:80:1: remark: Function Name: _ZN4mpcg11k_sched_keyElPKdPfPi [-Rpass-analysis=kernel-resource-usage]",
        "x.hip:80:1: remark:     VGPRs: 12 [-Rpass-analysis=kernel-resource-usage]",
    ])
    u = build.kernel_resources(text)
    k = "_ZN4mpcg12k_solve_wideILi0ELb1EdLi1ELb1EEEvNS_8WideArgsE"
    assert u[k] == {"VGPRs": 256, "ScratchSize [bytes/lane]": 128, "Occupancy [waves/SIMD]": 2,
                    "SGPRs Spill": 341, "LDS Size [bytes/block]": 4096}
    assert u["_ZN4mpcg11k_sched_keyElPKdPfPi"] == {"VGPRs": 12}


def test_parallel_build_units_cover_every_instance_group():
    """The parallel build compiles mpcg_wide_inst.hip once per group: the groups it names are
    exactly the groups of the instance list in wide_plan.h (a group without a unit would
    leave its kernels undefined at link time; a unit without instances is wasted), and every
    batch instance's (model, split, blocks) has an fp64 resume instance of its own kind (its
    parked problems, and the fp32 solver's escalations): the solve and warm instances among the
    RESUME rows, the per-problem ones among PP_RESUME, the started ones among START_RESUME."""
    import re

    from mpc_ros_amd import build

    text = open(os.path.join(build.CSRC, "wide_plan.h")).read()
    rows = re.findall(r"X\((\d+), ([A-Z_]+), (\d), (true|false), (double|float), (\d), (true|false), (\d)\)", text)
    resume_of = {"SOLVE": "RESUME", "WARM": "RESUME", "PP_SOLVE": "PP_RESUME", "START": "START_RESUME"}
    kinds = {r[1] for r in rows}
    assert kinds == set(resume_of) | set(resume_of.values())
    groups = {int(r[0]) for r in rows}
    units = [u for u in build.compile_units() if u[0] == build.INST]
    assert sorted(int(u[1][0].split("=")[1]) for u in units) == sorted(groups) == list(range(build.N_INST))
    for kind, rkind in resume_of.items():
        batch = [r for r in rows if r[1] == kind]
        res = {tuple(r[2:6]) for r in rows if r[1] == rkind}
        assert batch and res
        for _g, _k, m, sp, ty, nb, _d, _w in batch:
            # (the fp32 solver's problems that need the restoration phase are solved again by the
            # fp64 resume instance of the same horizon)
            assert (m, sp, "double", nb) in res, (kind, m, sp, nb)
    # every source of the library is compiled exactly once besides the instance groups
    others = [u[0] for u in build.compile_units() if u[0] != build.INST]
    assert sorted(others) == sorted(s for s in build.SOURCES if s != build.INST)


def test_launch_plan_native_check():
    """tests/native/wide_plan_check.cpp (mpc_ros_amd/csrc/wide_plan.h on the host, no GPU
    runtime): every key chosen by any of the seven key functions is a row of the instance list
    under its kind and every row is chosen by some input; the started kind's key is the plain
    general-options key; the workspace layout's regions are in order, aligned
    and disjoint for every horizon class, precision, park capacity and batch size, and so are the
    regions of a control tick's scratch (TickLayout) over B x Mmax x rows or none and of the host
    solve's staging (IoLayout) over B x N x rows, sol, start or none.  The solve
    instance it chooses over model x precision x N = 1..128 x default / non-default options x
    B in {1, 4096, 4097} equals the recorded choice of the dispatcher before the plan was a
    header (tests/golden/launch_plan.json), which holds the names the GPU tests pin."""
    import json
    import re
    import subprocess

    import host_harness
    from conftest import ROOT as root

    exe = host_harness.build("wide_plan_check", "-O1")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(root, "tests", "golden", "launch_plan.json")) as f:
        want = json.load(f)["instance_choice"]
    got = json.loads(r.stdout)
    assert len(want) == 24 and got == want
    names = {row[2] for rows in want.values() for row in rows}
    pinned = set()
    for mod in ("test_gpu_options.py", "test_gpu_headline.py"):
        text = open(os.path.join(root, "tests", mod)).read()
        pinned |= set(re.findall(r'"(k_solve_wide<[^"]*>)"', text))
    assert len(pinned) >= 3 and pinned <= names, pinned - names


def test_params_struct_bytes(libmpcg):
    """solver._params_struct adds nothing of its own to the library's defaults: without keywords
    its struct is the bytes mpcg_params_plugin_default / mpcg_params_default write (the plugin's
    are params.PLUGIN_DEFAULTS' values); "fp32" changes the fields of
    FP32_OPTIONS and no other; a keyword that is no field raises."""
    import ctypes as C

    from mpc_ros_amd import _lib, solver

    for base, default in (("plugin", libmpcg.mpcg_params_plugin_default), ("class", libmpcg.mpcg_params_default)):
        want = _lib.MpcgParams()
        assert default(C.byref(want)) == 0
        assert bytes(solver._params_struct(None, "fp64", {}, base=base)) == bytes(want)
    plugin = _lib.MpcgParams()
    assert libmpcg.mpcg_params_plugin_default(C.byref(plugin)) == 0
    assert bytes(solver._params_struct(None, "fp64", {})) == bytes(plugin)
    assert bytes(solver._params_struct(params.PLUGIN_DEFAULTS, "fp64", {})) == bytes(plugin)
    p32 = solver._params_struct(None, "fp32", {})
    differ = {n for n, _ in _lib.MpcgParams._fields_ if getattr(p32, n) != getattr(plugin, n)}
    # (no_restoration = 0 is FP32_OPTIONS' value and the default alike)
    assert differ == set(solver.FP32_OPTIONS) - {"no_restoration"}
    assert all(getattr(p32, k) == v for k, v in solver.FP32_OPTIONS.items())
    with pytest.raises(AttributeError):
        solver._params_struct(None, "fp64", {"no_such_option": 1})
