// mpc_ros_amd/csrc/mpcg_api.cpp -- the C-ABI of include/mpcg.h.
//
// Owns device buffers and a stream per handle; translates the reference's
// parameter map semantics (MPC::LoadParams / FG_eval::LoadParams,
// mpc_ros/src/mpc_planner.cpp:71-97, 243-262) into the kernel's IpmParams.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "mpcg.h"
#include "mpcg_internal.h"
#include "mpcg_kkt.h"
#include "mpcg_sens.h"
#include "mpcg_shift.h"
#include "mpcg_pp.h"
#include "mpcg_window.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace mpcg {
int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace mpcg

namespace {
int fail(int code, const std::string& msg) { return mpcg::set_error(code, msg); }
int hip_fail(hipError_t e, const char* what) {
    return fail(-2, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

// a device buffer of a handle: only ever grown (ensure)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <class T>
    T* at(const mpcg::Region& r) const {
        return (T*)((char*)p + r.off);
    }
};

struct mpcg_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    // the restoration phase's resume workers run on aux alongside the batch kernel (fork /
    // join events on the caller's stream)
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // (the fp32 configuration's head runs on aux, its resume workers on aux2)
    hipStream_t aux2 = nullptr;
    hipEvent_t ev_join2 = nullptr;
    mpcg_params params{};
    int strategy = MPCG_STRATEGY_AUTO;
    // The handle's device buffers (grown by ensure, freed by mpcg_destroy):
    //   io     staging of mpcg_solve's host arrays
    //   tick   a control tick's intermediates (wide_plan.h TickLayout)
    //   pp     preprocessing scratch of plans longer than 64 waypoints
    //   sched  solve-order buffers (keys, indices, sort scratch)
    //   spill  HBM workspace slots of the solver's rare paths and restoration phase
    DevBuf d_io, d_tick, d_pp, d_sched, d_spill;
    // stream ordering of the scratch above (with_scratch): the last stream that used it and an
    // event recorded after that use
    hipStream_t last_stream = nullptr;
    hipEvent_t last_ev = nullptr;
    bool have_last = false;
    // the solver kernel instance the last solve launched (mpcg_last_kernel)
    const char* last_kernel = "";
    // 1 if the last solve ran in expected-longest-first order (B > kOrderMinBatch)
    int last_ordered = 0;
    // park-area entries (0: the default, max(256, B / 128))
    int64_t park_cap = 0;
    // the synthetic robots' arc-length table (mpcg_synth_infinity_device), uploaded once
    double* d_arc = nullptr;
};

#ifndef MPCG_BUILD_ID
#define MPCG_BUILD_ID "unversioned"
#endif

extern "C" {

int mpcg_abi_version(void) { return MPCG_ABI_VERSION; }
const char* mpcg_build_id(void) {
    static const char kId[] = MPCG_BUILD_ID;  // "MPCG-BUILD-ID:<source hash>" (mpc_ros_amd/build.py)
    return std::strncmp(kId, "MPCG-BUILD-ID:", 14) == 0 ? kId + 14 : kId;
}
const char* mpcg_last_error(void) { return g_err.c_str(); }

// (the Ipopt options: ipm_core.h MPCG_IPOPT_OPTIONS)
static void ipopt_defaults(mpcg_params* p) {
#define MPCG_OPT_DEFAULT(type, field, name, dflt) p->name = dflt;
    MPCG_IPOPT_OPTIONS(MPCG_OPT_DEFAULT)
#undef MPCG_OPT_DEFAULT
    p->wheelbase = 0.5;
    p->model = 0;
    p->max_cpu_time = 0.5;  // mpc_planner.cpp:368
}

// max_cpu_time as the iterations the reference's Solve affords in that time at horizon
// N: CppAD taping 1.52 ms (N = 20) / 3.93 ms (N = 40) and derivative cost 0.225 / 0.467 ms
// per iteration, measured in the survey, plus Ipopt's own per-iteration
// work (KKT factorisation and solve, line search): the structured oracle's iteration on
// one EPYC 9575F core, 0.103 ms at N = 20 (profiles/r3/cpu_iter_cost.json), taken linear
// in N (5.14 us per stage).  0.5 s -> 1520 iterations at N = 20, 737 at N = 40.  -1: no
// budget.  (oracle/ipm.c ora_cpu_iter_budget restates the same model for the checker.)
static int cpu_iter_budget(double max_cpu_time, int steps) {
    if (!(max_cpu_time > 0) || max_cpu_time >= 999999.0) return -1;
    const double setup = std::fmax(0.0, 0.1205e-3 * steps - 0.89e-3);
    const double per = std::fmax(0.0121e-3 * steps - 0.017e-3, 1e-5) + 5.14e-6 * steps;
    const double b = std::floor((max_cpu_time - setup) / per);
    return b < 0 ? 0 : (b > 1e9 ? 1000000000 : (int)b);
}

int mpcg_params_default(mpcg_params* p) {
    if (!p) return fail(-1, "null params");
    std::memset(p, 0, sizeof *p);
    // MPC::MPC() (mpc_planner.cpp:223-241)
    p->steps = 20;
    p->max_angvel = 3.0;
    p->max_throttle = 1.0;
    p->bound = 1.0e3;
    // FG_eval::FG_eval (mpc_planner.cpp:42-68)
    p->dt = 0.1;
    p->ref_cte = 0.0;
    p->ref_etheta = 0.0;
    p->ref_v = 0.5;
    p->w_cte = 100;
    p->w_etheta = 100;
    p->w_v = 1;
    p->w_angvel = 100;
    p->w_accel = 50;
    p->w_angvel_d = 0;
    p->w_accel_d = 0;
    ipopt_defaults(p);
    return 0;
}

int mpcg_params_plugin_default(mpcg_params* p) {
    if (!p) return fail(-1, "null params");
    std::memset(p, 0, sizeof *p);
    // mpc_ros/cfg/MPCPlanner.cfg:22-37; DT = 1/controller_frequency (driving_state.cpp:28)
    p->steps = 20;
    p->dt = 0.1;
    p->ref_cte = 0.0;
    p->ref_etheta = 0.0;
    p->ref_v = 1.0;
    p->w_cte = 1000;
    p->w_etheta = 1000;
    p->w_v = 100;
    p->w_angvel = 100;
    p->w_accel = 50;
    p->w_angvel_d = 0;
    p->w_accel_d = 10;
    p->max_angvel = 1.0;
    p->max_throttle = 1.0;
    p->bound = 1000;
    ipopt_defaults(p);
    return 0;
}

int mpcg_params_set(mpcg_params* p, const char* key, double v) {
    if (!p || !key) return fail(-1, "null argument");
    const std::string k(key);
    if (k == "DT") p->dt = v;
    else if (k == "STEPS") p->steps = (int32_t)v;  // double -> int truncation, as the reference
    else if (k == "REF_CTE") p->ref_cte = v;
    else if (k == "REF_ETHETA") p->ref_etheta = v;
    else if (k == "REF_V") p->ref_v = v;
    else if (k == "W_CTE") p->w_cte = v;
    else if (k == "W_EPSI") p->w_etheta = v;
    else if (k == "W_V") p->w_v = v;
    else if (k == "W_ANGVEL") p->w_angvel = v;
    else if (k == "W_A") p->w_accel = v;
    else if (k == "W_DANGVEL") p->w_angvel_d = v;
    else if (k == "W_DA") p->w_accel_d = v;
    else if (k == "ANGVEL") p->max_angvel = v;
    else if (k == "MAXTHR") p->max_throttle = v;
    else if (k == "BOUND") p->bound = v;
    // extension keys (not in the reference map): dynamics model and wheelbase
    else if (k == "MODEL") p->model = (int32_t)v;
    else if (k == "LF") p->wheelbase = v;
    else return 1;
    return 0;
}

int mpcg_params_check(const mpcg_params* p) {
    if (!p) return fail(-1, "null params");
    if (p->steps < 2 || p->steps > 4096) return fail(-1, "STEPS must be in [2, 4096]");
    if (!(p->max_cpu_time > 0)) return fail(-1, "max_cpu_time must be > 0");
    if (p->acceptable_iter < 0 || p->max_soc < 0 || p->watchdog_shortened_iter_trigger < 0 ||
        p->watchdog_trial_iter_max < 0 || p->max_soft_resto_iters < 0 || p->max_filter_resets < 0 ||
        p->filter_reset_trigger < 1)
        return fail(-1, "invalid Ipopt integer option");
    if (!(p->soft_resto_pderror_reduction_factor >= 0) || !(p->tiny_step_tol >= 0) || !(p->kappa_soc > 0) ||
        !(p->dual_inf_tol > 0) || !(p->constr_viol_tol > 0) || !(p->compl_inf_tol > 0))
        return fail(-1, "invalid Ipopt option");
    if (!(p->dt > 0) || !std::isfinite(p->dt)) return fail(-1, "DT must be > 0");
    if (!(p->max_angvel > 0) || !(p->max_throttle > 0) || !(p->bound > 0)) return fail(-1, "bounds must be > 0");
    const double w[] = {p->w_cte, p->w_etheta, p->w_v, p->w_angvel, p->w_accel, p->w_angvel_d, p->w_accel_d};
    for (double x : w)
        if (!(x >= 0) || !std::isfinite(x)) return fail(-1, "weights must be finite and >= 0");
    if (!(p->tol > 0)) return fail(-1, "tol must be > 0");
    if (p->max_iter < 0) return fail(-1, "max_iter must be >= 0");
    if (p->filter_cap < 1 || p->filter_cap > 1024) return fail(-1, "filter_cap must be in [1, 1024]");
    if (!(p->bound_relax_factor >= 0) || !(p->mu_init > 0)) return fail(-1, "invalid Ipopt options");
    if (p->model != 0 && p->model != 1) return fail(-1, "model must be 0 (differential drive) or 1 (bicycle)");
    if (p->model == 1 && !(p->wheelbase > 0)) return fail(-1, "model 1 needs wheelbase (LF) > 0");
    if (p->precision != 0 && p->precision != 1) return fail(-1, "precision must be 0 (fp64) or 1 (fp32)");
    if (p->precision == 1 && p->model != 0) return fail(-1, "precision 1 (fp32) runs the differential drive only");
    if (p->no_restoration != 0 && p->no_restoration != 1) return fail(-1, "no_restoration must be 0 or 1");
    return 0;
}

static mpcg::IpmParams to_ipm(const mpcg_params& p) {
    mpcg::IpmParams q{};
    q.N = p.steps;
    q.dt = p.dt;
    q.ref_cte = p.ref_cte;
    q.ref_eth = p.ref_etheta;
    q.ref_v = p.ref_v;
    q.w_cte = p.w_cte;
    q.w_eth = p.w_etheta;
    q.w_v = p.w_v;
    q.w_w = p.w_angvel;
    q.w_a = p.w_accel;
    q.w_dw = p.w_angvel_d;
    q.w_da = p.w_accel_d;
    q.max_w = p.max_angvel;
    q.max_a = p.max_throttle;
    q.bound = p.bound;
    q.model = p.model;
    q.lf = p.wheelbase;
#define MPCG_OPT_COPY(type, field, name, dflt) q.field = p.name;
    MPCG_IPOPT_OPTIONS(MPCG_OPT_COPY)
#undef MPCG_OPT_COPY
    q.cpu_iter_budget = cpu_iter_budget(p.max_cpu_time, p.steps);
    q.precision = p.precision;
    return q;
}

// solve-order buffers (batches beyond the resident wavefronts)
using mpcg::kOrderMinBatch;
static mpcg::IpmParams handle_ipm(const mpcg_handle* h);

size_t mpcg_workspace_bytes(const mpcg_params* p, int64_t B) {
    if (!p || B <= 0) return 0;
    const mpcg::IpmParams P = to_ipm(*p);
    return mpcg::wide_spill_bytes(P, B) + (B > kOrderMinBatch ? mpcg::wide_sched_bytes(B) : 0);
}

// (the handle's own: its parameters, park capacity and device -- the slot partitions follow the
// device's XCD count)
size_t mpcg_handle_workspace_bytes(const mpcg_handle* h, int64_t B) {
    if (!h || B <= 0) return 0;
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != h->device;
    if (sw && hipSetDevice(h->device) != hipSuccess) return 0;
    const size_t n = mpcg::wide_spill_bytes(handle_ipm(h), B) + (B > kOrderMinBatch ? mpcg::wide_sched_bytes(B) : 0);
    if (sw) hipSetDevice(prev);
    return n;
}

int mpcg_create(int device, mpcg_handle** out) {
    if (!out) return fail(-1, "null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (device < 0 || device >= n) return fail(-3, "device ordinal out of range (no GPU?)");
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    mpcg_handle* h = new mpcg_handle();
    h->device = device;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return hip_fail(e, "hipStreamCreate");
    }
    mpcg_params_plugin_default(&h->params);
    e = hipEventCreateWithFlags(&h->last_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->aux2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join2, hipEventDisableTiming);
    if (e != hipSuccess) {
        mpcg_destroy(h);
        return hip_fail(e, "hipEventCreate / hipStreamCreate");
    }
    *out = h;
    return 0;
}

void mpcg_destroy(mpcg_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->have_last) hipEventSynchronize(h->last_ev);
    for (DevBuf* b : {&h->d_io, &h->d_tick, &h->d_pp, &h->d_sched, &h->d_spill})
        if (b->p) hipFree(b->p);
    if (h->d_arc) hipFree(h->d_arc);
    if (h->aux) hipStreamSynchronize(h->aux);
    if (h->aux2) hipStreamSynchronize(h->aux2);
    if (h->last_ev) hipEventDestroy(h->last_ev);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->ev_join2) hipEventDestroy(h->ev_join2);
    if (h->aux) hipStreamDestroy(h->aux);
    if (h->aux2) hipStreamDestroy(h->aux2);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int mpcg_set_params(mpcg_handle* h, const mpcg_params* p) {
    if (!h || !p) return fail(-1, "null argument");
    int rc = mpcg_params_check(p);
    if (rc) return rc;
    h->params = *p;
    return 0;
}

int mpcg_get_params(const mpcg_handle* h, mpcg_params* p) {
    if (!h || !p) return fail(-1, "null argument");
    *p = h->params;
    return 0;
}

static mpcg::IpmParams handle_ipm(const mpcg_handle* h) {
    mpcg::IpmParams P = to_ipm(h->params);
    P.park_cap = (int)h->park_cap;
    return P;
}

// Buffer b of at least `need` bytes.  One rule: nothing to do if it is large enough; otherwise
// the handle's device, a device synchronise only where an old buffer is freed (it may be in use on
// any stream), and the allocation.
static int ensure(mpcg_handle* h, DevBuf& b, size_t need, const char* what) {
    if (need <= b.bytes) return 0;
    hipSetDevice(h->device);
    if (b.p) {
        hipDeviceSynchronize();
        hipFree(b.p);
        b = DevBuf{};
    }
    hipError_t e = hipMalloc(&b.p, need);
    if (e != hipSuccess) {
        b.p = nullptr;
        return hip_fail(e, what);
    }
    b.bytes = need;
    return 0;
}

// the solver's scratch for a batch of B: the workspace slots and, for an ordered batch, the
// solve-order buffers
static int ensure_solve(mpcg_handle* h, int64_t B) {
    int rc = ensure(h, h->d_spill, mpcg::wide_spill_bytes(handle_ipm(h), B), "hipMalloc(spill areas)");
    if (rc || B <= kOrderMinBatch) return rc;
    return ensure(h, h->d_sched, mpcg::wide_sched_bytes(B), "hipMalloc(schedule buffers)");
}

// 160 KiB of LDS per CU: up to N = 64 a problem leaves room for a second wavefront (and
// eight fit at N = 20); up to N = 128 (two stage blocks) one problem may take the CU's LDS
static const size_t kWideLdsMax = 160 * 1024;

// The handle's scratch (solve order, spill areas, tick intermediates) is used stream-ordered:
// work queued on stream s first waits for the scratch's last use on another stream, and an event
// marks each use.  with_scratch is the one place that does both: `queue` launches the work, and
// whatever it returns -- also a failure after its first launch -- the use is recorded.
static int order_on(mpcg_handle* h, hipStream_t s) {
    if (h->have_last && h->last_stream != s) {
        hipError_t e = hipStreamWaitEvent(s, h->last_ev, 0);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    }
    return 0;
}
static int record_on(mpcg_handle* h, hipStream_t s) {
    hipError_t e = hipEventRecord(h->last_ev, s);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
    h->last_stream = s;
    h->have_last = true;
    return 0;
}
extern "C++" template <class Queue>  // (a template has C++ linkage, also in this block)
static int with_scratch(mpcg_handle* h, hipStream_t s, Queue&& queue) {
    int rc = order_on(h, s);
    if (rc) return rc;
    rc = queue();
    if (rc == 0) return record_on(h, s);
    const std::string err = g_err;  // (the failure's message, not the record's)
    record_on(h, s);
    return fail(rc, err);
}

static bool wave_fits(const mpcg::IpmParams& P) { return P.N <= 128 && mpcg::wide_lds_bytes(P) <= kWideLdsMax; }

// the prologue of the calls that take a handle and a batch
static int batch_check(const mpcg_handle* h, int64_t B) {
    if (!h) return fail(-1, "null handle");
    if (B < 0) return fail(-1, "negative batch");
    return 0;
}

int mpcg_reserve(mpcg_handle* h, int64_t B) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    return ensure_solve(h, B);
}

int mpcg_set_strategy(mpcg_handle* h, int32_t strategy) {
    if (!h) return fail(-1, "null handle");
    if (strategy == MPCG_STRATEGY_LANE) return fail(-1, "strategy LANE was removed in ABI 2 (one solver: WAVE)");
    if (strategy != MPCG_STRATEGY_AUTO && strategy != MPCG_STRATEGY_WAVE) return fail(-1, "unknown strategy");
    h->strategy = strategy;
    return 0;
}

int mpcg_get_strategy(const mpcg_handle* h) {
    if (!h) return fail(-1, "null handle");
    return MPCG_STRATEGY_WAVE;
}

int mpcg_solve_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, double* d_u0,
                      double* d_traj, int32_t* d_status, double* d_obj, int32_t* d_iters, void* stream) {
    return mpcg_solve_device_ex(h, B, d_state, d_coeffs, d_u0, d_traj, d_status, d_obj, d_iters, nullptr, stream);
}

static const char kNoFp32Rows[] =
    "precision 1 (fp32) takes no per-problem parameter rows: its fp64 phase and head have no per-problem instances";

// The refusals of a solve with the handle's parameters (rows: with a parameter row per problem),
// in two parts: the ticks check arguments of their own between them, in the order they always had
static int params_refusal(const mpcg_handle* h, bool rows) {
    int rc = mpcg_params_check(&h->params);
    if (rc) return rc;
    return rows && h->params.precision != 0 ? fail(-1, kNoFp32Rows) : 0;
}
static int lds_refusal(const mpcg_handle* h) {
    if (wave_fits(handle_ipm(h))) return 0;
    return fail(-1, "STEPS must be <= 128 (the problem state must fit the CU's 160 KiB of LDS)");
}

// Queues the solve of a request (device pointers) on s.  The caller has passed the refusals,
// grown the solver's scratch (ensure_solve) and ordered s (with_scratch).
static int queue_solve(mpcg_handle* h, const mpcg::SolveRequest& rq, hipStream_t s) {
    // batches larger than the resident wavefronts (8 per CU) are solved in
    // expected-longest-first order (launch_wide_order)
    int32_t* order = nullptr;
    if (rq.B > kOrderMinBatch) {
        hipError_t e = mpcg::launch_wide_order(rq.B, rq.coeffs, h->d_sched.p, h->d_sched.bytes, &order, s);
        if (e != hipSuccess) return hip_fail(e, "solve-order sort");
    }
    mpcg::WideStreams ws;
    ws.aux = h->aux;
    ws.aux2 = h->aux2;
    ws.ev_fork = h->ev_fork;
    ws.ev_join = h->ev_join;
    ws.ev_join2 = h->ev_join2;
    hipError_t e = mpcg::launch_wide_solve(handle_ipm(h), rq, order, h->d_spill.p, h->d_spill.bytes, s, ws,
                                           &h->last_kernel);
    if (e != hipSuccess) return hip_fail(e, "wide solve launch");
    h->last_ordered = order != nullptr;
    return 0;
}

static const char kNoFp32Sol[] =
    "precision 1 with no_restoration 1 (the fp32 phase alone) has no fp64 ending to report: no solution record";
static const char kNoFp32Start[] = "precision 1 (fp32) takes no start point: the started solve has fp64 instances only";

// The refusals of a solve request that the device and the host entries share, in their order
// (host: the arrays are the caller's own).  want_sol (mpcg_solve_device_sol, mpcg_solve_sol): the
// records are required.  1: nothing to do (B = 0).
static int request_refusal(const mpcg_handle* h, const mpcg::SolveRequest& rq, bool want_sol, bool host) {
    int rc = batch_check(h, rq.B);
    if (rc) return rc;
    if (want_sol && !rq.sol) return fail(-1, "sol is required");
    if (rq.started() && h->params.precision != 0) return fail(-1, kNoFp32Start);
    if (rq.B == 0) return 1;
    if (!rq.state || !rq.coeffs || !rq.u0) return fail(-1, "state, coeffs and u0 are required");
    // (fp32 with rows is refused before fp32 without an fp64 ending by the device entries, after it
    // by the host entries, which then read the rows: the order each always had)
    rc = params_refusal(h, !host && rq.rows);
    if (rc) return rc;
    if (want_sol && h->params.precision == 1 && h->params.no_restoration == 1) return fail(-1, kNoFp32Sol);
    if (!host || !rq.rows) return 0;
    if (h->params.precision != 0) return fail(-1, kNoFp32Rows);
    return mpcg_pparams_check(rq.rows, rq.B, h->params.model, nullptr);
}

// the device solve of a request, for every device entry
static int solve_device(mpcg_handle* h, const mpcg::SolveRequest& rq, void* stream, bool want_sol = false) {
    int rc = request_refusal(h, rq, want_sol, false);
    if (rc) return rc < 0 ? rc : 0;
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;  // NULL = the null stream, as in HIP
    rc = lds_refusal(h);
    if (rc == 0) rc = ensure_solve(h, rq.B);
    if (rc) return rc;
    return with_scratch(h, s, [&] { return queue_solve(h, rq, s); });
}

int mpcg_solve_device_ex(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, double* d_u0,
                         double* d_traj, int32_t* d_status, double* d_obj, int32_t* d_iters, int32_t* d_diag,
                         void* stream) {
    return solve_device(h, {B, d_state, d_coeffs, nullptr, d_u0, d_traj, d_status, d_obj, d_iters, d_diag}, stream);
}

int mpcg_solve_device_pp(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                         const double* d_pparams, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                         int32_t* d_iters, int32_t* d_diag, void* stream) {
    if (B > 0 && !d_pparams) return fail(-1, "pparams is required");
    return solve_device(h, {B, d_state, d_coeffs, d_pparams, d_u0, d_traj, d_status, d_obj, d_iters, d_diag}, stream);
}

int mpcg_solve_device_sol(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                          const double* d_pparams, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                          int32_t* d_iters, int32_t* d_diag, double* d_sol, void* stream) {
    return solve_device(h, {B, d_state, d_coeffs, d_pparams, d_u0, d_traj, d_status, d_obj, d_iters, d_diag, d_sol},
                        stream, true);
}

// ---- start point in ----
int mpcg_solve_device_start(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                            const double* d_pparams, const double* d_start, const int32_t* d_start_mode,
                            const double* d_mu0, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                            int32_t* d_iters, int32_t* d_diag, double* d_sol, int32_t* d_start_used, void* stream) {
    // (the start first: an argument check that needs no handle)
    if (!d_start || !d_start_mode) return fail(-1, "start and start_mode are required");
    return solve_device(h, {B, d_state, d_coeffs, d_pparams, d_u0, d_traj, d_status, d_obj, d_iters, d_diag, d_sol,
                            {d_start, d_start_mode, d_mu0, d_start_used}},
                        stream);
}

int64_t mpcg_solution_elems(int32_t N) { return N >= 2 ? mpcg::solution_elems(N) : 0; }

int mpcg_solve(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, double* u0, double* traj,
               int32_t* status, double* obj, int32_t* iters) {
    return mpcg_solve_ex(h, B, state, coeffs, u0, traj, status, obj, iters, nullptr);
}

// The host solve of a request whose arrays are the caller's own, for every host entry: staged
// through the handle's io block (wide_plan.h IoLayout), solved by solve_device on the handle's
// stream, copied back.  With a start the records are solved in place on the device: sol aliases
// the start records there.
static int solve_host(mpcg_handle* h, const mpcg::SolveRequest& host, bool want_sol = false) {
    int rc = request_refusal(h, host, want_sol, true);
    if (rc) return rc < 0 ? rc : 0;
    const int N = h->params.steps;
    const bool st = host.started();
    const mpcg::IoLayout L(host.B, N, host.rows != nullptr, host.sol != nullptr, st);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    rc = ensure(h, h->d_io, L.total, "hipMalloc(io)");
    if (rc) return rc;
    // (region, the caller's array in, the caller's array out, bytes: null arrays are not copied)
    struct Xfer {
        const mpcg::Region& r;
        const void* in;
        void* out;
        size_t bytes;
    };
    const size_t d = sizeof(double) * (size_t)host.B, i = sizeof(int32_t) * (size_t)host.B;
    const Xfer xfers[] = {{L.state, host.state, nullptr, 6 * d},
                          {L.coeffs, host.coeffs, nullptr, 4 * d},
                          {L.rows, host.rows, nullptr, MPCG_PP_FIELDS * d},
                          {L.rec, host.start.rec, host.sol, (size_t)mpcg::solution_elems(N) * d},
                          {L.mu0, host.start.mu0, nullptr, d},
                          {L.mode, host.start.mode, nullptr, i},
                          {L.u0, nullptr, host.u0, 2 * d},
                          {L.traj, nullptr, host.traj, 3 * (size_t)N * d},
                          {L.obj, nullptr, host.obj, d},
                          {L.status, nullptr, host.status, i},
                          {L.iters, nullptr, host.iters, i},
                          {L.diag, nullptr, host.diag, 4 * i},
                          {L.used, nullptr, host.start.used, i}};
    for (const Xfer& x : xfers)
        if (e == hipSuccess && x.in)
            e = hipMemcpyAsync(h->d_io.at<char>(x.r), x.in, x.bytes, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy H2D");
    const DevBuf& io = h->d_io;
    const mpcg::SolveRequest dev{host.B, io.at<double>(L.state), io.at<double>(L.coeffs),
                                 host.rows ? io.at<double>(L.rows) : nullptr, io.at<double>(L.u0),
                                 io.at<double>(L.traj), io.at<int32_t>(L.status), io.at<double>(L.obj),
                                 io.at<int32_t>(L.iters), host.diag ? io.at<int32_t>(L.diag) : nullptr,
                                 host.sol ? io.at<double>(L.rec) : nullptr,
                                 {st ? io.at<double>(L.rec) : nullptr, st ? io.at<int32_t>(L.mode) : nullptr,
                                  host.start.mu0 ? io.at<double>(L.mu0) : nullptr,
                                  st ? io.at<int32_t>(L.used) : nullptr}};
    rc = solve_device(h, dev, h->stream, want_sol);
    if (rc) return rc;
    for (const Xfer& x : xfers)
        if (e == hipSuccess && x.out)
            e = hipMemcpyAsync(x.out, h->d_io.at<char>(x.r), x.bytes, hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy D2H");
    e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return 0;
}

int mpcg_solve_start(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                     const double* start, const int32_t* start_mode, const double* mu0, double* u0, double* traj,
                     int32_t* status, double* obj, int32_t* iters, int32_t* diag, double* sol, int32_t* start_used) {
    if (!start || !start_mode) return fail(-1, "start and start_mode are required");
    return solve_host(h, {B, state, coeffs, pparams, u0, traj, status, obj, iters, diag, sol,
                          {start, start_mode, mu0, start_used}});
}

int mpcg_solve_sol(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                   double* u0, double* traj, int32_t* status, double* obj, int32_t* iters, int32_t* diag, double* sol) {
    return solve_host(h, {B, state, coeffs, pparams, u0, traj, status, obj, iters, diag, sol}, true);
}

// ---- the KKT certificate (mpcg_kkt.h) ----
int mpcg_kkt(const mpcg_params* p, int64_t B, const double* state, const double* coeffs, const double* pparams,
             const double* sol, double* cert) {
    if (!p) return fail(-1, "null params");
    if (B < 0) return fail(-1, "negative batch");
    if (B == 0) return 0;
    if (!state || !coeffs || !sol || !cert) return fail(-1, "state, coeffs, sol and cert are required");
    int rc = mpcg_params_check(p);
    if (rc) return rc;
    const mpcg::IpmParams P = to_ipm(*p);
    const mpcg::PPRow row = mpcg::pp_row_pack(P);
    const int64_t ne = mpcg::solution_elems(P.N);
    for (int64_t b = 0; b < B; ++b) {
        const mpcg::KktCert c = mpcg::kkt_problem(pparams ? pparams + b * MPCG_PP_FIELDS : row.f, P.model, P.N,
                                                  state + b * 6, coeffs + b * 4, sol + b * ne);
        cert[b * 4 + 0] = c.stat;
        cert[b * 4 + 1] = c.prim;
        cert[b * 4 + 2] = c.comp;
        cert[b * 4 + 3] = c.f;
    }
    return 0;
}

int mpcg_kkt_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, const double* d_pparams,
                    const double* d_sol, double* d_cert, void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    if (!d_state || !d_coeffs || !d_sol || !d_cert) return fail(-1, "state, coeffs, sol and cert are required");
    rc = mpcg_params_check(&h->params);
    if (rc) return rc;
    if (h->params.steps > 128) return fail(-1, "STEPS must be <= 128");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const mpcg::IpmParams P = handle_ipm(h);
    // (no handle scratch is touched: nothing to order against the handle's other streams)
    e = mpcg::launch_kkt_certify(B, P.N, P.model, mpcg::pp_row_pack(P), d_pparams, d_state, d_coeffs, d_sol, d_cert,
                                 (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "kkt certificate launch");
    return 0;
}

// ---- the shift rule (mpcg_shift.h) ----
int mpcg_shift_solution(const mpcg_params* p, int64_t B, const double* state, const double* coeffs,
                        const double* pparams, const double* motion, const int32_t* mask, const double* sol_in,
                        double* sol_out) {
    if (!p) return fail(-1, "null params");
    if (B < 0) return fail(-1, "negative batch");
    if (B == 0) return 0;
    if (!state || !coeffs || !motion || !sol_in || !sol_out)
        return fail(-1, "state, coeffs, motion, sol_in and sol_out are required");
    int rc = mpcg_params_check(p);
    if (rc) return rc;
    const mpcg::IpmParams P = to_ipm(*p);
    const mpcg::PPRow row = mpcg::pp_row_pack(P);
    const int64_t ne = mpcg::shift_record_elems(P.N);
    std::vector<double> work((size_t)ne);
    for (int64_t b = 0; b < B; ++b) {
        const double* in = sol_in + b * ne;
        double* out = sol_out + b * ne;
        if (mask && mask[b] == 0) {
            if (in != out) std::memmove(out, in, sizeof(double) * (size_t)ne);
            continue;
        }
        mpcg::shift_problem(pparams ? pparams + b * MPCG_PP_FIELDS : row.f, P.model, P.N, state + b * 6, coeffs + b * 4,
                            motion + b * 3, in, out, work.data());
    }
    return 0;
}

int mpcg_shift_solution_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                               const double* d_pparams, const double* d_motion, const int32_t* d_mask,
                               const double* d_sol_in, double* d_sol_out, void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    if (!d_state || !d_coeffs || !d_motion || !d_sol_in || !d_sol_out)
        return fail(-1, "state, coeffs, motion, sol_in and sol_out are required");
    rc = mpcg_params_check(&h->params);
    if (rc) return rc;
    if (h->params.steps > 128) return fail(-1, "STEPS must be <= 128");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const mpcg::IpmParams P = handle_ipm(h);
    // (no handle scratch is touched: nothing to order against the handle's other streams)
    e = mpcg::launch_shift_solution(B, P.N, P.model, mpcg::pp_row_pack(P), d_pparams, d_state, d_coeffs, d_motion, d_mask,
                                    d_sol_in, d_sol_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "shift launch");
    return 0;
}

// ---- the feedback gains (mpcg_sens.h) ----
int mpcg_sens(const mpcg_params* p, int64_t B, const double* state, const double* coeffs, const double* pparams,
              const double* sol, double* gain, double* dx, int32_t* info) {
    (void)state;  // (the gain does not depend on the bound of the initial-state rows)
    if (!p) return fail(-1, "null params");
    if (B < 0) return fail(-1, "negative batch");
    if (!sol || !gain) return fail(-1, "sol and gain are required");
    if (B == 0) return 0;
    if (!coeffs) return fail(-1, "coeffs is required");
    int rc = mpcg_params_check(p);
    if (rc) return rc;
    if (pparams && p->precision != 0) return fail(-1, kNoFp32Rows);
    const mpcg::IpmParams P = to_ipm(*p);
    const mpcg::PPRow row = mpcg::pp_row_pack(P);
    const int64_t ne = mpcg::solution_elems(P.N), nx = 8 * (int64_t)P.N - 2;
    std::vector<double> w((size_t)mpcg::sens_work_elems(P.N));
    mpcg::SensHostLanes ex;
    for (int64_t b = 0; b < B; ++b) {
        const int e = mpcg::sens_problem(ex, w.data(), pparams ? pparams + b * MPCG_PP_FIELDS : row.f, P.model, P.N,
                                         P.constr_viol_tol, P.bound_relax_factor, coeffs + b * 4, sol + b * ne,
                                         gain + b * 2 * MPCG_SENS_COLS, dx ? dx + b * MPCG_SENS_COLS * nx : nullptr);
        if (info) info[b] = e;
    }
    return 0;
}

int mpcg_sens_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, const double* d_pparams,
                     const double* d_sol, double* d_gain, double* d_dx, int32_t* d_info, void* stream) {
    (void)d_state;
    int rc = batch_check(h, B);
    if (rc) return rc;
    if (!d_sol || !d_gain) return fail(-1, "sol and gain are required");
    if (B == 0) return 0;
    if (!d_coeffs) return fail(-1, "coeffs is required");
    rc = mpcg_params_check(&h->params);
    if (rc) return rc;
    if (d_pparams && h->params.precision != 0) return fail(-1, kNoFp32Rows);
    if (h->params.steps > 128) return fail(-1, "STEPS must be <= 128");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const mpcg::IpmParams P = handle_ipm(h);
    // (the work area is the kernel's LDS at every horizon: no handle scratch, nothing to order)
    e = mpcg::launch_sens(B, P.N, P.model, mpcg::pp_row_pack(P), P.constr_viol_tol, P.bound_relax_factor, d_pparams,
                          d_coeffs, d_sol, d_gain, d_dx, d_info, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "sensitivity launch");
    return 0;
}

int mpcg_sens_apply(const mpcg_params* p, int64_t B, const double* pparams, const double* gain, const double* u0,
                    const double* dstate, const double* dcoeffs, double* u) {
    if (!p) return fail(-1, "null params");
    if (B < 0) return fail(-1, "negative batch");
    if (B == 0) return 0;
    if (!gain || !u0 || !dstate || !u) return fail(-1, "gain, u0, dstate and u are required");
    const mpcg::PPRow row = mpcg::pp_row_pack(to_ipm(*p));
    for (int64_t b = 0; b < B; ++b)
        mpcg::sens_apply(pparams ? pparams + b * MPCG_PP_FIELDS : row.f, gain + b * 2 * MPCG_SENS_COLS, u0 + b * 2,
                         dstate + b * 6, dcoeffs ? dcoeffs + b * 4 : nullptr, u + b * 2);
    return 0;
}

int mpcg_sens_apply_device(mpcg_handle* h, int64_t B, const double* d_pparams, const double* d_gain, const double* d_u0,
                           const double* d_dstate, const double* d_dcoeffs, double* d_u, void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    if (!d_gain || !d_u0 || !d_dstate || !d_u) return fail(-1, "gain, u0, dstate and u are required");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = mpcg::launch_sens_apply(B, mpcg::pp_row_pack(handle_ipm(h)), d_pparams, d_gain, d_u0, d_dstate, d_dcoeffs, d_u,
                                (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "sensitivity apply launch");
    return 0;
}

int mpcg_solve_ex(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, double* u0, double* traj,
                  int32_t* status, double* obj, int32_t* iters, int32_t* diag) {
    return solve_host(h, {B, state, coeffs, nullptr, u0, traj, status, obj, iters, diag});
}

int mpcg_solve_pp(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                  double* u0, double* traj, int32_t* status, double* obj, int32_t* iters, int32_t* diag) {
    if (B > 0 && !pparams) return fail(-1, "pparams is required");
    return solve_host(h, {B, state, coeffs, pparams, u0, traj, status, obj, iters, diag});
}

int mpcg_pparams_fill(const mpcg_params* p, int64_t B, double* rows) {
    if (!p || !rows) return fail(-1, "null argument");
    if (B < 0) return fail(-1, "negative batch");
    double row[MPCG_PP_FIELDS];
    mpcg::pp_row_from(to_ipm(*p), row);
    for (int64_t b = 0; b < B; ++b) std::memcpy(rows + b * MPCG_PP_FIELDS, row, sizeof row);
    return 0;
}

int mpcg_pparams_check(const double* rows, int64_t B, int32_t model, int64_t* bad_row) {
    if (!rows && B > 0) return fail(-1, "null rows");
    if (B < 0) return fail(-1, "negative batch");
    if (model != 0 && model != 1) return fail(-1, "model must be 0 (differential drive) or 1 (bicycle)");
    for (int64_t b = 0; b < B; ++b)
        if (!mpcg::pp_row_ok(rows + b * MPCG_PP_FIELDS, model)) {
            if (bad_row) *bad_row = b;
            return fail(-1, "parameter row " + std::to_string(b) +
                                ": every value finite, DT, ANGVEL, MAXTHR, BOUND > 0, weights >= 0" +
                                (model == 1 ? ", LF > 0" : ""));
        }
    return 0;
}

double mpcg_decelerate(double dist, double v, double max_throttle, double max_speed, double min_speed, double ref_v) {
    return mpcg::decelerate(dist, v, max_throttle, max_speed, min_speed, ref_v);
}

// ---- the control tick: preprocessing, solve, post-processing ----

// findBestPath returns without solving for an empty plan (driving_state.cpp:182-185);
// polyfit asserts order 3 <= M - 1 (:286); any longer plan is taken (beyond 64
// waypoints through an HBM workspace)
static const char kShortPlan[] = "M (waypoints per robot) must be >= 4";

// the preprocessing scratch of a plan of M waypoints for every robot (none up to 64)
static int ensure_pp(mpcg_handle* h, int64_t B, int M) {
    return ensure(h, h->d_pp, mpcg::find_best_path_ws_bytes(B, M), "hipMalloc(preprocessing scratch)");
}
// Queues findBestPath's preprocessing on s, for mpcg_preprocess_device(_n) and the tick.  d_count
// null: M waypoints for every robot, any M >= 4 (beyond 64 through the scratch, which the caller
// has grown: ensure_pp); else d_count[b] waypoints for robot b in plan rows of M <= 64.
static int queue_preprocess(mpcg_handle* h, int64_t B, int M, const int32_t* d_count, const double* d_pose,
                            const double* d_vel, const double* d_plan, int delay_mode, double* d_state,
                            double* d_coeffs, hipStream_t s) {
    hipError_t e = mpcg::launch_find_best_path(B, M, d_count, h->params.dt, delay_mode ? 1 : 0, d_pose, d_vel, d_plan,
                                               d_state, d_coeffs, (double*)h->d_pp.p, s);
    return e == hipSuccess ? 0 : hip_fail(e, "find_best_path launch");
}

int mpcg_preprocess_device(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                           const double* d_plan, int32_t delay_mode, double* d_state, double* d_coeffs,
                           void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    if (M < 4) return fail(-1, kShortPlan);
    if (!d_pose || !d_vel || !d_plan || !d_state || !d_coeffs) return fail(-1, "null buffer");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_pp(h, B, M);
    if (rc) return rc;
    auto queue = [&] { return queue_preprocess(h, B, M, nullptr, d_pose, d_vel, d_plan, delay_mode, d_state, d_coeffs, s); };
    // (up to 64 waypoints it touches none of the handle's scratch)
    return mpcg::find_best_path_ws_bytes(B, M) ? with_scratch(h, s, queue) : queue();
}

// The start of a warm tick (mpcg_rollout_device_start): the caller's carry and what decides its use
struct WarmTick {
    int start_mode;         // MPCG_START_*, uniform
    double mu0;             // FULL's barrier parameter
    const int32_t* done;    // [B] (after the tick's done mark)
    double* carry_sol;      // [B][solution_elems(N)] in/out
    double* carry_pose;     // [B][3] in/out
    int32_t* carry_ok;      // [B] in/out
    int32_t* used;          // [B] the mode that ran, or null
};
// One tick's inputs and outputs (device pointers)
static_assert(mpcg::kRowFields == MPCG_PP_FIELDS, "TickLayout's rows are parameter rows");
struct Tick {
    int64_t B;
    int M;                 // plan rows per robot
    const double* pose;    // [B][3]
    const double* vel;     // [B][3]
    const double* plan;    // [B][M][2]
    const int32_t* count;  // [B] robot b's waypoints in its M rows, or null: M for every robot
    int delay_mode;
    const double* rows;    // [B][16] a parameter row per robot, or null: the handle's parameters
    const double* ref_v;   // [B] the speed clamp of each robot, or null: the handle's REF_V
    double* cmd;           // [B][3]
    double* traj;          // [B][3][N], or null
    int32_t* status;       // [B], or null
    int32_t* iters;        // [B], or null
    const WarmTick* warm = nullptr;  // the tick started from the carried records, or null
};

// Everything a call of ticks allocates, before its first launch: the tick scratch of layout L,
// the preprocessing scratch of a uniform plan of M waypoints (0: a count per robot) and the solver's
static int ensure_tick(mpcg_handle* h, const mpcg::TickLayout& L, int64_t B, int M) {
    int rc = ensure(h, h->d_tick, L.total, "hipMalloc(track buffers)");
    if (rc == 0) rc = ensure_pp(h, B, M);
    return rc ? rc : ensure_solve(h, B);
}

// Queues one tick on s: the three stages through the scratch regions of L.  The caller has passed
// the refusals, called ensure_tick and ordered s (with_scratch).  Rows or none, the solver's
// instance follows: k_solve_wide_pp or k_solve_wide.
static int tick(mpcg_handle* h, const Tick& t, const mpcg::TickLayout& L, hipStream_t s) {
    double *st = h->d_tick.at<double>(L.state), *cf = h->d_tick.at<double>(L.coeffs), *u0 = h->d_tick.at<double>(L.u0);
    int rc = queue_preprocess(h, t.B, t.M, t.count, t.pose, t.vel, t.plan, t.delay_mode, st, cf, s);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (const WarmTick* w = t.warm) {
        // the carried records shifted in place to this tick's frame, then the started solve in
        // place on them (every robot without a usable record in COLD mode)
        int32_t *mode = h->d_tick.at<int32_t>(L.mode), *status = t.status ? t.status : h->d_tick.at<int32_t>(L.status);
        double* mu0 = h->d_tick.at<double>(L.mu0);
        e = mpcg::launch_shift_rollout(t.B, h->params.steps, h->params.model, w->start_mode, w->mu0, t.rows, st, cf,
                                       t.pose, w->done, w->carry_ok, w->carry_pose, w->carry_sol, mode, mu0, s);
        if (e != hipSuccess) return hip_fail(e, "shift launch");
        rc = queue_solve(h, {t.B, st, cf, t.rows, u0, t.traj, status, nullptr, t.iters, nullptr, w->carry_sol,
                             {w->carry_sol, mode, mu0, w->used}}, s);
        if (rc) return rc;
        e = mpcg::launch_carry_flag(t.B, w->done, status, w->carry_ok, s);
        if (e != hipSuccess) return hip_fail(e, "carry flag launch");
    } else {
        rc = queue_solve(h, {t.B, st, cf, t.rows, u0, t.traj, t.status, nullptr, t.iters}, s);
        if (rc) return rc;
    }
    e = mpcg::launch_post(t.B, h->params.dt, h->params.ref_v, t.ref_v, t.vel, u0, t.cmd, s);
    return e == hipSuccess ? 0 : hip_fail(e, "post-processing launch");
}

int mpcg_track_device(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                      const double* d_plan, int32_t delay_mode, double* d_cmd, double* d_traj, int32_t* d_status,
                      void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    if (!d_cmd) return fail(-1, "cmd is required");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (M < 4) return fail(-1, kShortPlan);
    if (!d_pose || !d_vel || !d_plan) return fail(-1, "null buffer");
    rc = params_refusal(h, false);
    if (rc == 0) rc = lds_refusal(h);
    const mpcg::TickLayout L(B, 0, 0);
    if (rc == 0) rc = ensure_tick(h, L, B, M);
    if (rc) return rc;
    const Tick t{B, M, d_pose, d_vel, d_plan, nullptr, delay_mode, nullptr, nullptr, d_cmd, d_traj, d_status, nullptr};
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(h, s, [&] { return tick(h, t, L, s); });
}

static const char kSpeedsFinite[] = "max_speed and min_speed must be finite";

int mpcg_track_device_goal(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                           const double* d_plan, const double* d_goal, double* d_ref_v, double max_speed,
                           double min_speed, int32_t delay_mode, double* d_cmd, double* d_traj, int32_t* d_status,
                           void* stream) {
    int rc = batch_check(h, B);
    if (rc || B == 0) return rc;
    // (every refusal before the first launch: deceleration rewrites ref_v)
    if (M < 4) return fail(-1, kShortPlan);
    if (!d_cmd || !d_goal || !d_ref_v || !d_pose || !d_vel || !d_plan)
        return fail(-1, "cmd, goal, ref_v, pose, vel and plan are required");
    rc = params_refusal(h, true);
    if (rc) return rc;
    if (!std::isfinite(max_speed) || !std::isfinite(min_speed)) return fail(-1, kSpeedsFinite);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    rc = lds_refusal(h);
    const mpcg::TickLayout L(B, 0, 1);
    if (rc == 0) rc = ensure_tick(h, L, B, M);
    if (rc) return rc;
    double* rows = h->d_tick.at<double>(L.rows);
    const Tick t{B, M, d_pose, d_vel, d_plan, nullptr, delay_mode, rows, d_ref_v, d_cmd, d_traj, d_status, nullptr};
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(h, s, [&] {
        e = mpcg::launch_decelerate(B, d_pose, d_vel, d_goal, d_ref_v, mpcg::decel_throttle(h->params.max_throttle),
                                    max_speed, min_speed, mpcg::pp_row_pack(to_ipm(h->params)), rows, s);
        return e == hipSuccess ? tick(h, t, L, s) : hip_fail(e, "deceleration launch");
    });
}

// ---- the closed loop on the device ----

// Mmax = ceil(window_wp / stride) + 1 of a plan window's arguments
static int window_mmax(int32_t window_wp, int32_t stride, int64_t* Mmax) {
    if (window_wp < 1 || stride < 1) return fail(-1, "window_wp and stride must be >= 1");
    *Mmax = mpcg::plan_window_mmax(window_wp, stride);
    return 0;
}

int32_t mpcg_plan_window_mmax(int32_t window_wp, int32_t stride) {
    int64_t m = 0;
    const int rc = window_mmax(window_wp, stride, &m);
    if (rc) return rc;
    if (m > INT32_MAX) return fail(-1, "Mmax = ceil(window_wp / stride) + 1 exceeds int32");
    return (int32_t)m;
}

int mpcg_plan_window(const double* course, int32_t G, int32_t cursor, double x, double y, int32_t window_wp,
                     int32_t stride, int32_t* new_cursor, int32_t* start, int32_t* count, double* plan) {
    if (!course || !plan) return fail(-1, "course and plan are required");
    if (G < 1) return fail(-1, "G (course waypoints) must be >= 1");
    if (cursor < 0 || cursor >= G) return fail(-1, "cursor must be in [0, G)");
    const int32_t m = mpcg_plan_window_mmax(window_wp, stride);
    if (m < 0) return m;
    const mpcg::PlanWindow w = mpcg::plan_window(course, G, cursor, x, y, window_wp, stride);
    mpcg::plan_window_copy(course, w, stride, m, plan);
    if (new_cursor) *new_cursor = w.cursor;
    if (start) *start = w.start;
    if (count) *count = w.count;
    return 0;
}

// the window arguments the device calls share; *Mmax on success
static int window_args_check(int32_t C, int32_t Gmax, int32_t window_wp, int32_t stride, int* Mmax) {
    int64_t m = 0;
    const int rc = window_mmax(window_wp, stride, &m);
    if (rc) return rc;
    if (C < 1 || Gmax < 1) return fail(-1, "C (courses) and Gmax (waypoints per course) must be >= 1");
    if (m > mpcg::kWindowMaxM)
        return fail(-1, "Mmax = ceil(window_wp / stride) + 1 must be <= 64 (sampled waypoints per robot)");
    *Mmax = (int)m;
    return 0;
}

int mpcg_plan_window_device(mpcg_handle* h, int64_t B, const double* d_courses, const int32_t* d_course_len,
                            const int32_t* d_course_of, int32_t C, int32_t Gmax, const double* d_pose,
                            int32_t window_wp, int32_t stride, int32_t* d_cursor, double* d_plan, int32_t* d_count,
                            void* stream) {
    int rc = batch_check(h, B);
    if (rc) return rc;
    int Mmax = 0;
    rc = window_args_check(C, Gmax, window_wp, stride, &Mmax);
    if (rc || B == 0) return rc;
    if (!d_courses || !d_course_len || !d_course_of || !d_pose || !d_cursor || !d_plan || !d_count)
        return fail(-1, "null buffer");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = mpcg::launch_plan_window(B, d_courses, d_course_len, d_course_of, C, Gmax, d_pose, window_wp, stride, Mmax,
                                 d_cursor, d_plan, d_count, nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "plan window launch");
    return 0;
}

int mpcg_preprocess_device_n(mpcg_handle* h, int64_t B, int32_t Mmax, const double* d_pose, const double* d_vel,
                             const double* d_plan, const int32_t* d_count, int32_t delay_mode, double* d_state,
                             double* d_coeffs, void* stream) {
    int rc = batch_check(h, B);
    if (rc) return rc;
    if (Mmax < 1 || Mmax > mpcg::kWindowMaxM) return fail(-1, "Mmax (plan rows per robot) must be in [1, 64]");
    if (B == 0) return 0;
    if (!d_pose || !d_vel || !d_plan || !d_count || !d_state || !d_coeffs) return fail(-1, "null buffer");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return queue_preprocess(h, B, Mmax, d_count, d_pose, d_vel, d_plan, delay_mode, d_state, d_coeffs,
                            (hipStream_t)stream);
}

// The rollout, cold (warm null: mpcg_rollout_device) or started from the caller's carry
// (mpcg_rollout_device_start; log_used [K][B] or null)
static int rollout(mpcg_handle* h, int64_t B, int32_t K, const double* d_courses, const int32_t* d_course_len,
                   const int32_t* d_course_of, int32_t C, int32_t Gmax, int32_t window_wp, int32_t stride,
                   double goal_tol, double max_speed, double min_speed, int32_t delay_mode, int32_t integrate,
                   double* d_pose, double* d_vel, int32_t* d_cursor, double* d_ref_v, int32_t* d_done,
                   const mpcg_rollout_logs* logs, void* stream, WarmTick* warm, int32_t* log_used) {
    int rc = batch_check(h, B);
    if (rc) return rc;
    // (every refusal before the first launch: a tick rewrites the robots' state)
    if (K < 1) return fail(-1, "K (ticks) must be >= 1");
    int Mmax = 0;
    rc = window_args_check(C, Gmax, window_wp, stride, &Mmax);
    if (rc == 0) rc = params_refusal(h, true);
    if (rc) return rc;
    if (!std::isfinite(max_speed) || !std::isfinite(min_speed)) return fail(-1, kSpeedsFinite);
    if (std::isnan(goal_tol)) return fail(-1, "goal_tol must be a number");
    if (warm) {
        // (PRIMAL is not offered here: inside the rollout's kernel sequence a PRIMAL-started solve
        // did not repeat bit for bit from call to call, and K ticks in one call must equal K calls)
        if (warm->start_mode == MPCG_START_PRIMAL)
            return fail(-1, "start_mode MPCG_START_PRIMAL is not offered by the rollout: MPCG_START_COLD or _FULL");
        if (warm->start_mode != MPCG_START_COLD && warm->start_mode != MPCG_START_FULL)
            return fail(-1, "start_mode must be MPCG_START_COLD or MPCG_START_FULL");
        if (warm->start_mode == MPCG_START_FULL && !(warm->mu0 > 0 && std::isfinite(warm->mu0)))
            return fail(-1, "mu0 must be positive and finite in FULL mode");
    }
    if (B == 0) return 0;
    if (!d_courses || !d_course_len || !d_course_of || !d_pose || !d_vel || !d_cursor || !d_ref_v || !d_done)
        return fail(-1, "courses, course_len, course_of, pose, vel, cursor, ref_v and done are required");
    if (warm && (!warm->carry_sol || !warm->carry_pose || !warm->carry_ok))
        return fail(-1, "carry_sol, carry_pose and carry_ok are required");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    rc = lds_refusal(h);
    const mpcg::TickLayout L(B, Mmax, 1, warm ? 1 : 0);
    if (rc == 0) rc = ensure_tick(h, L, B, 0);
    if (rc) return rc;
    double *rows = h->d_tick.at<double>(L.rows), *cmd = h->d_tick.at<double>(L.cmd), *plan = h->d_tick.at<double>(L.plan);
    int32_t *count = h->d_tick.at<int32_t>(L.count), *start = h->d_tick.at<int32_t>(L.start);
    const mpcg::PPRow row = mpcg::pp_row_pack(to_ipm(h->params));
    const mpcg_rollout_logs lg = logs ? *logs : mpcg_rollout_logs{};
    Tick t{B, Mmax, d_pose, d_vel, plan, count, delay_mode, rows, d_ref_v, cmd, nullptr, nullptr, nullptr, warm};
    mpcg::RolloutArgs a{};  // (what no tick changes: all but the tick's index and its rows of the logs)
    a.B = B;
    a.courses = d_courses;
    a.course_len = d_course_len;
    a.course_of = d_course_of;
    a.C = C;
    a.Gmax = Gmax;
    a.goal_tol = goal_tol;
    a.max_throttle = mpcg::decel_throttle(h->params.max_throttle);
    a.max_speed = max_speed;
    a.min_speed = min_speed;
    a.dt = h->params.dt;
    a.integrate = integrate ? 1 : 0;
    a.pose = d_pose;
    a.vel = d_vel;
    a.cursor = d_cursor;
    a.start = start;
    a.count = count;
    a.ref_v = d_ref_v;
    a.done = d_done;
    a.rows = rows;
    a.cmd = cmd;
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(h, s, [&] {
        for (int32_t k = 0; k < K; ++k) {
            // this tick's row of a log of w values per robot (null stays null)
            auto at = [&](auto* log, int w) { return log ? log + (size_t)w * k * (size_t)B : nullptr; };
            e = mpcg::launch_plan_window(B, d_courses, d_course_len, d_course_of, C, Gmax, d_pose, window_wp, stride,
                                         Mmax, d_cursor, plan, count, start, s);
            if (e != hipSuccess) return hip_fail(e, "plan window launch");
            a.tick = k;
            a.log_pose = at(lg.pose, 3);
            a.log_vel = at(lg.vel, 3);
            a.log_cmd = at(lg.cmd, 3);
            a.log_ref_v = at(lg.ref_v, 1);
            a.log_cursor = at(lg.cursor, 1);
            a.log_start = at(lg.start, 1);
            a.log_count = at(lg.count, 1);
            e = mpcg::launch_rollout_begin(a, row, s);
            if (e != hipSuccess) return hip_fail(e, "rollout tick launch");
            t.status = at(lg.status, 1);
            t.iters = at(lg.iters, 1);
            if (warm) warm->used = at(log_used, 1);
            rc = tick(h, t, L, s);
            if (rc) return rc;
            e = mpcg::launch_rollout_end(a, s);
            if (e != hipSuccess) return hip_fail(e, "rollout tick launch");
        }
        return 0;
    });
}

int mpcg_rollout_device(mpcg_handle* h, int64_t B, int32_t K, const double* d_courses, const int32_t* d_course_len,
                        const int32_t* d_course_of, int32_t C, int32_t Gmax, int32_t window_wp, int32_t stride,
                        double goal_tol, double max_speed, double min_speed, int32_t delay_mode, int32_t integrate,
                        double* d_pose, double* d_vel, int32_t* d_cursor, double* d_ref_v, int32_t* d_done,
                        const mpcg_rollout_logs* logs, void* stream) {
    return rollout(h, B, K, d_courses, d_course_len, d_course_of, C, Gmax, window_wp, stride, goal_tol, max_speed,
                   min_speed, delay_mode, integrate, d_pose, d_vel, d_cursor, d_ref_v, d_done, logs, stream, nullptr,
                   nullptr);
}

int mpcg_rollout_device_start(mpcg_handle* h, int64_t B, int32_t K, const double* d_courses,
                              const int32_t* d_course_len, const int32_t* d_course_of, int32_t C, int32_t Gmax,
                              int32_t window_wp, int32_t stride, double goal_tol, double max_speed, double min_speed,
                              int32_t delay_mode, int32_t integrate, double* d_pose, double* d_vel, int32_t* d_cursor,
                              double* d_ref_v, int32_t* d_done, const mpcg_rollout_logs* logs, void* stream,
                              int32_t start_mode, double mu0, double* d_carry_sol, double* d_carry_pose,
                              int32_t* d_carry_ok, int32_t* d_log_start_used) {
    WarmTick w{start_mode, mu0, d_done, d_carry_sol, d_carry_pose, d_carry_ok, nullptr};
    return rollout(h, B, K, d_courses, d_course_len, d_course_of, C, Gmax, window_wp, stride, goal_tol, max_speed,
                   min_speed, delay_mode, integrate, d_pose, d_vel, d_cursor, d_ref_v, d_done, logs, stream, &w,
                   d_log_start_used);
}

const char* mpcg_last_kernel(const mpcg_handle* h) { return h ? h->last_kernel : ""; }
int mpcg_last_solve_order(const mpcg_handle* h) { return h ? h->last_ordered : 0; }

int mpcg_synth_infinity_device(mpcg_handle* h, uint64_t seed, int64_t start, int64_t B, int32_t M, double* d_pose,
                               double* d_vel, double* d_plan, void* stream) {
    if (!h) return fail(-1, "null handle");
    if (B < 0 || start < 0) return fail(-1, "negative batch or start");
    if (B == 0) return 0;
    if (M < 4) return fail(-1, "M (waypoints per robot) must be >= 4");
    if (!d_pose || !d_vel || !d_plan) return fail(-1, "null buffer");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const int n = mpcg::synth_arc_len();
    if (!h->d_arc) {
        std::vector<double> t, s;
        mpcg::synth_arc_table(t, s);
        e = hipMalloc((void**)&h->d_arc, sizeof(double) * 2 * n);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(arc table)");
        e = hipMemcpy(h->d_arc, t.data(), sizeof(double) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(h->d_arc + n, s.data(), sizeof(double) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(h->d_arc);
            h->d_arc = nullptr;
            return hip_fail(e, "hipMemcpy(arc table)");
        }
    }
    e = mpcg::launch_synth_infinity(seed, start, B, M, h->d_arc, h->d_arc + n, d_pose, d_vel, d_plan,
                                    (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "synthetic robots launch");
    return 0;
}

int mpcg_set_park_capacity(mpcg_handle* h, int64_t cap) {
    if (!h) return fail(-1, "null handle");
    if (cap < 0 || cap > (int64_t)1 << 30) return fail(-1, "park capacity must be in [0, 2^30]");
    h->park_cap = cap;
    return 0;
}

int mpcg_synchronize(mpcg_handle* h) {
    if (!h) return fail(-1, "null handle");
    hipSetDevice(h->device);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return 0;
}

}  // extern "C"
