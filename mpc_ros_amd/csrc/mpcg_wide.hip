// mpc_ros_amd/csrc/mpcg_wide.hip -- one problem per wavefront (wide_core.h) on CDNA4: the
// launch side (solve order, the instance table, batch kernel + resume workers).  What to launch
// and where in the workspace is wide_plan.h (instance choice, workspace layout: no runtime
// calls); the kernels are in mpcg_wide_kern.h, their instances in mpcg_wide_inst.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <utility>
#include <hipcub/device/device_radix_sort.hpp>

#include "mpcg_wide_kern.h"

namespace mpcg {

// Scheduling key: workgroups are dispatched roughly in index order, so a slow problem
// dispatched late extends the launch (its iterations run at the lone-wavefront rate
// after the rest of the batch is done).  The curvature of the reference polynomial
// predicts the slow tail (infinity set: 36 of the 39 problems above p99 in iterations
// are in the top decile of |c1| + |c2| + |c3|), so problems are solved in descending
// order of it.  Results do not depend on the order.
__global__ void __launch_bounds__(256) k_sched_key(int64_t B, const double* coeffs, float* key, int32_t* idx) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    const double* c = coeffs + p * 4;
    key[p] = (float)(fabs(c[1]) + fabs(c[2]) + fabs(c[3]));
    idx[p] = (int32_t)p;
}

// the workspace's per-launch state: the slot flags, the 64 counters (park count / taken / done /
// started, the overflow count / taken), the park ready flags, the overflow list (-1: not yet
// published)
__global__ void __launch_bounds__(256) k_reset_ws(int32_t* flags, int64_t nflags, int32_t* cnt, int32_t* pready,
                                                  int64_t npready, int64_t* ovf, int64_t novf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nflags) flags[i] = 0;
    if (i < 64) cnt[i] = 0;
    if (i < npready) pready[i] = 0;
    if (i < novf) ovf[i] = -1;
}

size_t wide_sched_bytes(int64_t B) {
    size_t temp = 0;
    hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, (const float*)nullptr, (float*)nullptr,
                                                 (const int32_t*)nullptr, (int32_t*)nullptr, (int)B);
    return 2 * sizeof(float) * B + 2 * sizeof(int32_t) * B + temp + 256;
}

hipError_t launch_wide_order(int64_t B, const double* coeffs, void* buf, size_t bytes, int32_t** order,
                             hipStream_t stream) {
    char* b = (char*)buf;
    float* k0 = (float*)b;
    float* k1 = k0 + B;
    int32_t* v0 = (int32_t*)(k1 + B);
    int32_t* v1 = v0 + B;
    void* temp = (void*)(((uintptr_t)(v1 + B) + 255) & ~(uintptr_t)255);
    size_t temp_bytes = bytes - ((char*)temp - b);
    hipLaunchKernelGGL(k_sched_key, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, coeffs, k0, v0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, k0, k1, v0, v1, (int)B, 0, 32, stream);
    *order = v1;
    return e;
}

// The kernels of wide_plan.h's rows, row by row: filled once, by every group's wide_group
// (mpcg_wide_inst.hip).  A diagnostic build with MPCG_HEADLINE_ONLY links only the benchmark
// configuration's groups, 0 and 1 (tools/build_wt.sh): every other row stays null.
#ifdef MPCG_HEADLINE_ONLY
constexpr int kLinkedGroups = 2;
#else
constexpr int kLinkedGroups = kWideGroups;
#endif
template <int... G>
static void fill_groups(const void** t, std::integer_sequence<int, G...>) {
    (wide_group<G>(t), ...);
}
// the instance of a key; fn null: the key is none (refused parameters) or not in the library
static WideInst find_inst(const WideKey& k) {
    static const void* const* table = [] {
        static const void* t[kWideInstances] = {};
        fill_groups(t, std::make_integer_sequence<int, kLinkedGroups>());
        return t;
    }();
    const int i = k.ok() ? find_key(k) : -1;
    return i < 0 ? WideInst{nullptr, "", k.kind} : WideInst{table[i], kWideNames[i], k.kind};
}
WideInst wide_kernel(int kind, const IpmParams& P, int64_t B) {
    return find_inst(kind == PP_SOLVE ? pp_solve_key(P, B) : kind == START ? start_key(P) : solve_key(P, B));
}

// XCDs of the current device (HW_REG_XCC_ID partitions of the workspace slots); 8 on an
// MI355X in SPX mode, fewer on a partitioned device
static int device_xccs() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess ||
        n < 1)
        return kXcds;
    return n > 16 ? 16 : n;
}
// A phase's slot budget (wide_plan.h slot_count): four times the wavefronts the device can hold
// resident at once -- occupancy of the batch instance at its LDS size times the CUs
static int64_t slot_budget(const IpmParams& P, int64_t B) {
    const void* fn = wide_kernel(SOLVE, P, B).fn;
    const size_t lds = wide_lds_bytes(P);
    int dev = 0, cus = 0, per = 0;
    if (fn && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, 64, lds) == hipSuccess && per > 0 && cus > 0)
        return 4 * (int64_t)per * cus;
    return 4096;  // (fallback if the runtime cannot say)
}
// the workspace of a solve on the current device: what only the runtime can say, asked once
static SolveLayout solve_layout(const IpmParams& P, int64_t B) { return SolveLayout(P, B, device_xccs(), slot_budget); }
size_t wide_spill_bytes(const IpmParams& P, int64_t B) { return solve_layout(P, B).total; }

// diag[p][2] = mark for the problems p = order[0, K) (of n_prob)
__global__ void __launch_bounds__(256) k_mark_rows(int64_t K, const int32_t* order, int32_t* diag, int32_t mark,
                                                   int64_t n_prob) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= K) return;
    const int64_t p = order[b];
    check_index("head order: problem", p, n_prob);
    diag[p * 4 + 2] = mark;
}

// The fp64 phase's solve order: the problems the fp32 phase did not converge on (solved from the
// start: full-length fp64 solves, some through the restoration phase) first, then the others (a
// few fp64 iterations each), so the long solves do not trail the batch.  Positions by two atomic
// counters (from the front, and from the back): results do not depend on the order.
__global__ void __launch_bounds__(256) k_cold_first(int64_t B, const float* h, int64_t stride, const int32_t* order,
                                                    int32_t* out, int32_t* cnt, int64_t n_prob) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int32_t p = order ? order[b] : (int32_t)b;
    check_index("fp64 phase order: problem", p, n_prob);
    if (h[(int64_t)p * stride] != 0.0f)
        out[B - 1 - atomicAdd(&cnt[1], 1)] = p;
    else
        out[atomicAdd(&cnt[0], 1)] = p;
}

// Concurrent resume workers (parked problems in flight while the batch kernel runs): each
// holds a wavefront slot and a problem's LDS for the whole batch kernel (32 workers cost
// the batch kernel ~7 %, 2 under 1 %), and problems park rarely (~5e-5 of the infinity set
// at N = 20, ~5e-4 at N = 40; ~4e-3 with the fp32 solver): two, and one more per 65536
// problems.  What is still parked when the batch ends goes to the drain launch.
#ifndef MPCG_RESUME_WORKERS
#define MPCG_RESUME_WORKERS 2
#endif
// (MPCG_RESUME_WORKERS in the environment overrides the count: a tuning knob, read once)
static int64_t resume_workers(int64_t B) {
    static const int64_t env = [] {
        const char* s = getenv("MPCG_RESUME_WORKERS");
        return s ? (int64_t)atoll(s) : (int64_t)-1;
    }();
    return env > 0 ? env : MPCG_RESUME_WORKERS + B / 65536;
}
// One batch launch (with its resume workers, drain and overflow launches) of a solve request (its
// arrays are shared by every phase: rq.B problems, the caller's batch): the instance inst for
// parameters P, on B problems in the given order, on the workspace `lay` at base.  The kind of
// inst says what the kernels take after WideArgs -- PP_SOLVE: the request's rows, START: its
// start as StartIn (which carries the rows) -- and which resume instance continues it.  handoff: the
// fp32 configuration's hand-over buffer (the fp32 phase writes it, the fp64 phase -- inst a
// k_warm_wide instance -- reads it).  nworkers: concurrent resume workers (0: resume_workers).
// origin (the fp32 configuration's head): &the caller's stream (a pointer: the caller's stream may
// be the null stream) -- the workspace reset runs there, then both `stream` and (with workers)
// `aux` fork from it (ev_fork), and the caller joins them; no stream forks from a forked
// stream, which a captured graph does not survive.
struct PhaseLaunch {
    IpmParams P;
    WideInst inst;
    int64_t B = 0;
    const int32_t* order = nullptr;
    const PhaseLayout* lay = nullptr;
    char* base = nullptr;
    float* handoff = nullptr;
    int64_t handoff_stride = 0;
    hipStream_t stream = nullptr, aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int64_t nworkers = 0;
    const hipStream_t* origin = nullptr;
};
// the solver addresses its dynamic LDS from address 0 (wave_dev.h): no static LDS
static hipError_t set_dynamic_lds(const void* fn, size_t lds) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, fn);
    if (e != hipSuccess) return e;
    if (fa.sharedSizeBytes != 0) return hipErrorInvalidKernelFile;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
// `into` continues after what `from` holds so far
static hipError_t join(hipEvent_t ev, hipStream_t from, hipStream_t into) {
    const hipError_t e = hipEventRecord(ev, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(into, ev, 0);
}
// (*forked_out: whether aux received work)
static hipError_t launch_phase(const SolveRequest& rq, const PhaseLaunch& L, bool* forked_out = nullptr) {
    const IpmParams& P = L.P;
    const PhaseLayout& W = *L.lay;
    size_t lds = wide_lds_bytes(P);
#ifdef MPCG_LDS_PAD_ENV
    // (diagnostic builds only: extra LDS per workgroup, fewer problems per CU)
    if (const char* pad = getenv("MPCG_LDS_PAD")) lds += (size_t)atol(pad);
#endif
    const void* fn = L.inst.fn;
    if (!fn) return hipErrorInvalidValue;
    const bool fp32_phase = P.precision == 1 && L.handoff;  // (parks nothing: its endings go to the hand-over)
    const void* rf = fp32_phase ? nullptr : find_inst(resume_key_of(L.inst.kind, P)).fn;
    if (!fp32_phase && !rf) return hipErrorInvalidValue;
    // (every host-side call before the first launch: the device does not wait for the host
    // between the reset kernel and the solver -- ~15 us of a B = 1 solve otherwise)
    hipError_t e = set_dynamic_lds(fn, lds);
    if (e == hipSuccess && rf) e = set_dynamic_lds(rf, lds);
    if (e != hipSuccess) return e;
    const int64_t B = L.B, ns = W.nslots, pc = W.park_cap, nov = W.has_ovf() ? B : 0;
    int32_t* cnt = (int32_t*)(L.base + W.counters.off);
    WideArgs a{.P = P, .B = B, .order = L.order, .state = rq.state, .coeffs = rq.coeffs, .u0 = rq.u0, .traj = rq.traj,
               .status = rq.status, .obj = rq.obj, .iters = rq.iters, .diag = rq.diag, .n_prob = rq.B,
               .slots = L.base + W.slots.off, .slot_flags = (int32_t*)(L.base + W.flags.off), .nslots = (int32_t)ns,
               .slot_elems = (int32_t)W.slot_elems, .park_count = cnt + PhaseLayout::PARK_COUNT,
               .park_cap = fp32_phase ? 0 : (int32_t)pc, .park_idx = (int64_t*)(L.base + W.park_idx.off),
               .park_ready = (int32_t*)(L.base + W.park_ready.off), .park_taken = cnt + PhaseLayout::PARK_TAKEN,
               .done = cnt + PhaseLayout::DONE, .park = L.base + W.park.off, .park_stride = W.park_stride,
               .started = cnt + PhaseLayout::STARTED, .ovf_count = cnt + PhaseLayout::OVF_COUNT,
               .ovf_taken = cnt + PhaseLayout::OVF_TAKEN, .ovf_idx = (int64_t*)(L.base + W.ovf.off),
               .nxcc = (int32_t)W.nxcc, .phase = 0, .ent0 = 0, .ovf_mark = 2, .handoff = L.handoff,
               .handoff_stride = L.handoff ? L.handoff_stride : 0, .sol = rq.sol,
               .sol_stride = solution_elems(P.N)};
    // (the per-problem kernels take the rows as a second argument, after WideArgs; the started
    // solve's kernels take StartIn there instead; the other kinds read no second argument)
    const double* rows = rq.rows;
    const StartIn si{rq.start.rec, solution_elems(P.N), rq.start.mode, rq.start.mu0, rq.start.used, rq.rows};
    void* second = L.inst.kind == START ? (void*)&si : (void*)&rows;
    void* args[] = {(void*)&a, second};
    // the resume workers: parked problems (the restoration phase) continued by k_resume_wide
    // fork: the resume workers on the aux stream alongside the batch kernel (the fork point is
    // before the batch kernel); join: the stream continues after both (no host
    // synchronisation).  Under graph capture the two branches need not run concurrently: the
    // workers then exit at once (take_parked) and the drain takes every parked problem.  No
    // worker, no fork (a captured fork whose branch held no work deadlocked the second replay of
    // the graph).
    const int64_t nw = L.nworkers > 0 ? L.nworkers : resume_workers(B);
    // (B = 1: a parked problem is the whole batch, the drain continues it as soon as a worker
    // would -- no fork, no worker spinning beside the solve)
    const bool can_fork = !fp32_phase && B > 1 && L.aux && L.aux != L.stream && L.ev_fork && L.ev_join;
    const unsigned workers = can_fork ? (unsigned)(pc < nw ? pc : nw) : 0u;
    const bool fork = workers > 0;
    if (forked_out) *forked_out = fork;
    // (the per-launch state -- slot flags, counters, park ready flags, the overflow list at -1 --
    // reset by a kernel, not by memset nodes: a captured graph replayed a second time ran its
    // small memsets unordered with the solver kernels)
    const hipStream_t from = L.origin ? *L.origin : L.stream;  // (where the streams of this launch fork from)
    {
        int64_t n = pc > 64 ? pc : 64;
        n = n > nov ? n : nov;
        n = n > ns ? n : ns;
        hipLaunchKernelGGL(k_reset_ws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, from, a.slot_flags, ns, cnt,
                           a.park_ready, pc, a.ovf_idx, nov);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (L.origin || fork) {
        e = hipEventRecord(L.ev_fork, from);
        if (e == hipSuccess && L.origin) e = hipStreamWaitEvent(L.stream, L.ev_fork, 0);
        if (e == hipSuccess && fork) e = hipStreamWaitEvent(L.aux, L.ev_fork, 0);
        if (e != hipSuccess) return e;
    }
    e = hipLaunchKernel(fn, dim3((unsigned)B), dim3(64), args, lds, L.stream);
    if (fp32_phase) return e != hipSuccess ? e : hipGetLastError();
    if (e != hipSuccess) return e;
    if (fork) {
        e = hipLaunchKernel(rf, dim3(workers), dim3(64), args, lds, L.aux);
        if (e != hipSuccess) return e;
    }
    // the drain, after the batch kernel: one worker per park entry, so the problems still
    // waiting when the batch ends run side by side (a worker finding nothing left exits at once)
    // -- the tail is the longest restoration, not their sum over a few workers
    e = hipLaunchKernel(rf, dim3((unsigned)pc), dim3(64), args, lds, L.stream);
    if (e != hipSuccess) return e;
    if (fork && !L.origin) {  // (with an origin the caller joins both streams there)
        e = join(L.ev_join, L.aux, L.stream);
        if (e != hipSuccess) return e;
    }
    // the park-area overflow (only where it can occur: pc < B), after every worker that holds a
    // park entry: problems solved again from the start, one per park entry at a time
    if (W.has_ovf()) {
        WideArgs ao = a;
        ao.phase = 1;
        void* oargs[] = {(void*)&ao, second};
        e = hipLaunchKernel(rf, dim3((unsigned)pc), dim3(64), oargs, lds, L.stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

hipError_t launch_wide_solve(const IpmParams& P, const SolveRequest& pb, const int32_t* order, void* spill,
                             size_t spill_bytes, hipStream_t stream, const WideStreams& ws,
                             const char** kernel_name) {
    const int64_t B = pb.B;
    if (B <= 0) return hipSuccess;
    if (!spill) return hipErrorInvalidValue;
    const SolveLayout W = solve_layout(P, B);
    if (W.total > spill_bytes) return hipErrorInvalidValue;
    // (per-problem rows: the same workspace -- the per-problem instance has its plain twin's LDS
    // size and register allocation, so the slot budget is the plain instance's)
    // (a started solve: the rows travel in StartIn; fp64 only -- start_key)
    PhaseLaunch L{.P = P, .inst = wide_kernel(pb.started() ? START : pb.rows ? PP_SOLVE : SOLVE, P, B), .B = B,
                  .order = order, .lay = &W.first, .base = (char*)spill, .stream = stream, .aux = ws.aux,
                  .ev_fork = ws.ev_fork, .ev_join = ws.ev_join};
    if (!L.inst.fn) return hipErrorInvalidValue;
    if (pb.started() && (W.two || !pb.start.rec || !pb.start.mode)) return hipErrorInvalidValue;
    if (pb.rows && W.two) return hipErrorInvalidValue;  // (the fp32 configuration: refused, wide_plan.h pp_solve_key)
    if (kernel_name) *kernel_name = L.inst.name;
    if (!W.two) return launch_phase(pb, L);
    // the fp32 configuration: [the head on aux, in fp64 from the start] the fp32 phase (hand-over,
    // no outputs), then the fp64 phase, over the problems outside the head
    const IpmParams Pr = fp64_params(P);
    const bool can_head = order && ws.aux && ws.aux != stream && ws.aux2 && ws.aux2 != ws.aux &&
                          ws.aux2 != stream && ws.ev_fork && ws.ev_join && ws.ev_join2;
    const int64_t K = can_head ? W.head_n : 0, Bm = B - K;
    // (with a head the two phases cover B - K problems: their layouts for that count, in the
    // space the workspace reserves for B)
    const PhaseLayout lay32 = K > 0 ? PhaseLayout(P, Bm, slot_budget(P, Bm), W.first.nxcc) : W.first;
    const PhaseLayout lay64 = K > 0 ? PhaseLayout(Pr, Bm, slot_budget(Pr, Bm), W.first.nxcc) : W.second;
    if (lay32.total > W.phases || lay64.total > W.phases) return hipErrorInvalidValue;
    hipError_t e;
    bool head_workers = false;
    if (K > 0) {
        // (after the solve order: the head is order[0, K), on its own workspace; aux and the
        // head's resume workers on aux2 both fork from the caller's stream -- no fork of a forked
        // stream, which a captured graph does not survive -- and both join it after the fp32 phase)
        PhaseLaunch H = L;
        H.P = head_params(P, K);
        H.inst = wide_kernel(SOLVE, H.P, B);  // (the fp64 solver's batch instance)
        H.B = K;
        H.lay = &W.head;
        H.base = (char*)spill + W.head_off;
        H.stream = ws.aux;
        H.aux = ws.aux2;
        H.ev_join = ws.ev_join2;
        H.origin = &stream;
        e = launch_phase(pb, H, &head_workers);
        if (e != hipSuccess) return e;
    }
    L.B = Bm;
    L.order = order ? order + K : nullptr;
    L.lay = &lay32;
    L.handoff = (float*)((char*)spill + W.handoff.off);
    L.handoff_stride = W.handoff_stride;
    e = launch_phase(pb, L);
    if (e != hipSuccess) return e;
    if (K > 0) {  // (the head joins before the fp64 phase forks its own workers onto aux)
        e = head_workers ? join(ws.ev_join2, ws.aux2, stream) : hipSuccess;
        if (e == hipSuccess) e = join(ws.ev_join, ws.aux, stream);
        if (e != hipSuccess) return e;
        if (pb.diag) {  // (solved from the start by the fp64 solver: diag[:, 2] = 3, after the head's last write)
            hipLaunchKernelGGL(k_mark_rows, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, K, order, pb.diag, 3, B);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    int32_t* order2 = (int32_t*)((char*)spill + W.order2.off);
    int32_t* cnt2 = (int32_t*)((char*)spill + W.cnt2.off);
    hipLaunchKernelGGL(k_reset_ws, dim3(1), dim3(256), 0, stream, cnt2, (int64_t)0, cnt2, nullptr, (int64_t)0,
                       nullptr, (int64_t)0);
    hipLaunchKernelGGL(k_cold_first, dim3((unsigned)((Bm + 255) / 256)), dim3(256), 0, stream, Bm,
                       (const float*)L.handoff, L.handoff_stride, L.order, order2, cnt2, B);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (the problems solved from the start come first and some of them enter the restoration
    // phase early in the launch: more concurrent resume workers than a batch of the fp64 solver
    // needs, so they are continued while the rest of the batch runs)
    L.P = Pr;
    L.inst = find_inst(warm_key(Pr));
    L.order = order2;
    L.lay = &lay64;
    L.nworkers = 8 + B / 2048;
    return launch_phase(pb, L);
}

}  // namespace mpcg
