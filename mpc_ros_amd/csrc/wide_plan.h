// mpc_ros_amd/csrc/wide_plan.h -- the launch plan of the wavefront solver (mpcg_wide.hip), as
// plain arithmetic on (IpmParams, B, slot budget, XCD count): the kernel instances the library
// carries and the choice among them, the layout of the HBM workspace, and the layout of a control
// tick's scratch and of a host solve's staging (TickLayout, IoLayout).  No GPU runtime: the
// launch side passes in what only the runtime can say (the occupancy behind the slot budget,
// the XCD count), and tests/native/wide_plan_check.cpp checks all of it on the host.
#ifndef MPCG_WIDE_PLAN_H
#define MPCG_WIDE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <cstdlib>

#include "wide_core.h"

// The instances the library carries, one row each:
//   X(group, kind, model, split, type, blocks, default options, waves per SIMD)
// group: the MPCG_INST translation unit that compiles it (mpcg_wide_inst.hip); kind: a WideKind
// below -- which kernel, and which key function chooses among the rows of the kind.  A resume row
// carries no options and no allocation of its own (false, 0: k_resume_wide reads the options and
// is always allocated for one wavefront per SIMD).
//   SOLVE         k_solve_wide (solve_key).
//   RESUME        k_resume_wide<RESUME> (resume_key).  The fp32 solver's problems that need the
//                 restoration phase are solved again in fp64: its resume kernel is the fp64
//                 instance of the same horizon.
//   WARM          k_warm_wide, the fp64 phase of the fp32 configuration, default options: per
//                 horizon class (warm_key).
//   PP_SOLVE      k_solve_wide_pp, a parameter row per problem (include/mpcg.h MPCG_PP_*;
//                 mpcg_solve_device_pp): general options, fp64, one per (model, horizon class)
//                 -- and the default-options instance of the benchmark class (pp_solve_key).
//   PP_RESUME     k_resume_wide<PP_RESUME> (pp_resume_key).
//   START         k_start_wide, a solve started from a solution record (include/mpcg.h
//                 mpcg_solve_device_start): general options, fp64, one per (model, horizon class)
//                 -- a parameter row per problem or none is a run-time argument of the one
//                 instance (start_key).
//   START_RESUME  k_resume_wide<START_RESUME>, whose overflow re-solve starts from the record
//                 again (start_resume_key).
// A new kind: an enumerator, its rows (in groups of their own), its kernel (or its branch of
// k_resume_wide) with the kernel's line in mpcg_wide_inst.hip, its name below, its key function.
#define MPCG_WIDE_INSTANCES(X)                        \
    X(0, SOLVE, 0, true, double, 1, true, 2)          \
    X(0, SOLVE, 0, true, double, 1, true, 1)          \
    X(1, SOLVE, 0, true, double, 1, false, 2)         \
    X(2, SOLVE, 0, false, double, 1, false, 2)        \
    X(2, SOLVE, 0, false, double, 1, false, 1)        \
    X(5, SOLVE, 0, false, double, 1, true, 2)         \
    X(3, SOLVE, 0, false, double, 2, false, 1)        \
    X(1, SOLVE, 0, false, double, 2, true, 1)         \
    X(6, SOLVE, 0, false, double, 1, true, 1)         \
    X(4, SOLVE, 0, true, float, 1, false, 3)          \
    X(5, SOLVE, 0, false, float, 1, false, 3)         \
    X(6, SOLVE, 0, false, float, 2, false, 2)         \
    X(7, SOLVE, 1, true, double, 1, false, 2)         \
    X(4, SOLVE, 1, true, double, 1, true, 2)          \
    X(8, SOLVE, 1, false, double, 1, false, 2)        \
    X(7, SOLVE, 1, false, double, 1, true, 2)         \
    X(8, SOLVE, 1, false, double, 1, false, 1)        \
    X(9, SOLVE, 1, false, double, 2, false, 1)        \
    X(1, RESUME, 0, true, double, 1, false, 0)        \
    X(2, RESUME, 0, false, double, 1, false, 0)       \
    X(3, RESUME, 0, false, double, 2, false, 0)       \
    X(7, RESUME, 1, true, double, 1, false, 0)        \
    X(8, RESUME, 1, false, double, 1, false, 0)       \
    X(9, RESUME, 1, false, double, 2, false, 0)       \
    X(10, WARM, 0, true, double, 1, true, 2)          \
    X(10, WARM, 0, false, double, 1, true, 2)         \
    X(11, WARM, 0, false, double, 1, true, 1)         \
    X(11, WARM, 0, false, double, 2, true, 1)         \
    X(12, PP_SOLVE, 0, true, double, 1, false, 2)     \
    X(19, PP_SOLVE, 0, true, double, 1, true, 2)      \
    X(13, PP_SOLVE, 0, false, double, 1, false, 2)    \
    X(14, PP_SOLVE, 0, false, double, 1, false, 1)    \
    X(14, PP_SOLVE, 0, false, double, 2, false, 1)    \
    X(15, PP_SOLVE, 1, true, double, 1, false, 2)     \
    X(16, PP_SOLVE, 1, false, double, 1, false, 2)    \
    X(17, PP_SOLVE, 1, false, double, 1, false, 1)    \
    X(18, PP_SOLVE, 1, false, double, 2, false, 1)    \
    X(12, PP_RESUME, 0, true, double, 1, false, 0)    \
    X(13, PP_RESUME, 0, false, double, 1, false, 0)   \
    X(15, PP_RESUME, 0, false, double, 2, false, 0)   \
    X(16, PP_RESUME, 1, true, double, 1, false, 0)    \
    X(17, PP_RESUME, 1, false, double, 1, false, 0)   \
    X(18, PP_RESUME, 1, false, double, 2, false, 0)   \
    X(20, START, 0, true, double, 1, false, 2)        \
    X(21, START, 0, false, double, 1, false, 2)       \
    X(22, START, 0, false, double, 1, false, 1)       \
    X(23, START, 0, false, double, 2, false, 1)       \
    X(24, START, 1, true, double, 1, false, 2)        \
    X(25, START, 1, false, double, 1, false, 2)       \
    X(26, START, 1, false, double, 1, false, 1)       \
    X(27, START, 1, false, double, 2, false, 1)       \
    X(28, START_RESUME, 0, true, double, 1, false, 0) \
    X(29, START_RESUME, 0, false, double, 1, false, 0) \
    X(30, START_RESUME, 0, false, double, 2, false, 0) \
    X(31, START_RESUME, 1, true, double, 1, false, 0) \
    X(32, START_RESUME, 1, false, double, 1, false, 0) \
    X(33, START_RESUME, 1, false, double, 2, false, 0)
// (an instance's name: mpcg_last_kernel() reports the batch kernel a solve launched)
#define MPCG_NAME6(k, M, S, T, NB, D, W) k "<" #M "," #S "," #T "," #NB "," #D "," #W ">"
#define MPCG_NAME4(k, M, S, T, NB, D, W) k #M "," #S "," #T "," #NB ">"
#define MPCG_NAME_SOLVE(...) MPCG_NAME6("k_solve_wide", __VA_ARGS__)
#define MPCG_NAME_WARM(...) MPCG_NAME6("k_warm_wide", __VA_ARGS__)
#define MPCG_NAME_PP_SOLVE(...) MPCG_NAME6("k_solve_wide_pp", __VA_ARGS__)
#define MPCG_NAME_START(...) MPCG_NAME6("k_start_wide", __VA_ARGS__)
#define MPCG_NAME_RESUME(...) MPCG_NAME4("k_resume_wide<RESUME,", __VA_ARGS__)
#define MPCG_NAME_PP_RESUME(...) MPCG_NAME4("k_resume_wide<PP_RESUME,", __VA_ARGS__)
#define MPCG_NAME_START_RESUME(...) MPCG_NAME4("k_resume_wide<START_RESUME,", __VA_ARGS__)

namespace mpcg {

// batches beyond the resident wavefronts are solved in expected-longest-first order
constexpr int64_t kOrderMinBatch = 2048;
constexpr int kXcds = 8;  // (MI355X; the runtime's count is used where it can say: device_xccs)

inline size_t round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }
inline size_t elem_bytes(const IpmParams& P) { return P.precision == 1 ? sizeof(float) : sizeof(double); }
// LDS bytes per problem
inline size_t wide_lds_bytes(const IpmParams& P) {
    return (size_t)WideLayout(P.N, P.filter_cap, P.model).total() * elem_bytes(P);
}

// ---------------------------------------------------------------- the instances and the choice
enum WideKind { SOLVE, RESUME, WARM, PP_SOLVE, PP_RESUME, START, START_RESUME };
// An instance's kind and template arguments (a resume instance: model, split, blocks; the rest
// zero).  model < 0: none -- the parameters are refused.
struct WideKey {
    int kind = SOLVE, model = -1;
    bool split = false, f32 = false;
    int nb = 0;
    bool defopt = false;
    int wpe = 0;
    bool ok() const { return model >= 0; }
    bool operator==(const WideKey& o) const {
        return kind == o.kind && model == o.model && split == o.split && f32 == o.f32 && nb == o.nb &&
               defopt == o.defopt && wpe == o.wpe;
    }
};
// the list as keys, names and groups, row by row (host side: the device code names no instance)
#define MPCG_ROW_KEY(g, K, M, S, T, NB, D, W) WideKey{K, M, S, sizeof(T) == 4, NB, D, W},
#define MPCG_ROW_NAME(g, K, M, S, T, NB, D, W) MPCG_NAME_##K(M, S, T, NB, D, W),
#define MPCG_ROW_GROUP(g, K, M, S, T, NB, D, W) g,
inline constexpr WideKey kWideKeys[] = {MPCG_WIDE_INSTANCES(MPCG_ROW_KEY)};
inline constexpr const char* kWideNames[] = {MPCG_WIDE_INSTANCES(MPCG_ROW_NAME)};
inline constexpr int kWideGroupOf[] = {MPCG_WIDE_INSTANCES(MPCG_ROW_GROUP)};
#undef MPCG_ROW_KEY
#undef MPCG_ROW_NAME
#undef MPCG_ROW_GROUP
constexpr int kWideInstances = (int)(sizeof(kWideKeys) / sizeof(kWideKeys[0]));
// the translation units of mpcg_wide_inst.hip: groups 0 .. kWideGroups - 1 (build.py N_INST)
constexpr int kWideGroups = [] {
    int n = 0;
    for (int g : kWideGroupOf) n = g + 1 > n ? g + 1 : n;
    return n;
}();
// the row of a key, -1: the library carries no such instance
inline int find_key(const WideKey& k) {
    for (int i = 0; i < kWideInstances; ++i)
        if (kWideKeys[i] == k) return i;
    return -1;
}

// The horizon class of a problem: SPLIT (N <= 32: the recursions use both half-waves), NB stage
// blocks (2 for 64 < N <= 128), and `one`: an fp64 problem of more than 32 KB of LDS (N >= 35;
// every N > 64) leaves room for at most 4 problems per CU (160 KB), one wavefront per SIMD --
// its instance is register-allocated for one (512 VGPRs, no spills) instead of two.  (A split
// problem is never `one`: its instances are allocated for two.)  Refused (ok = false): more
// than 128 stages, and the fp32 solver on anything but the differential drive.
struct WideClass {
    bool ok, split, one;
    int model, nb;
};
inline WideClass wide_class(const IpmParams& P) {
    WideClass c;
    c.ok = P.N <= 128 && !(P.precision == 1 && P.model != 0);
    c.model = P.model == 1 ? 1 : 0;
    c.split = P.N <= 32;
    c.nb = P.N > 64 ? 2 : 1;
    c.one = c.nb == 2 || (!c.split && wide_lds_bytes(P) > 32768);
    return c;
}

// A small batch (B <= kLoneBatch) runs the benchmark configuration's instance allocated for
// one wavefront per SIMD as well: its time is set by its longest problem at the
// lone-wavefront rate, which the 512-VGPR allocation (no spills) shortens (B = 4,096, the
// BASELINE's configs[1]: 3.02 -> 2.93 ms; B = 1,024 is held at one wavefront per SIMD).
constexpr int64_t kLoneBatch = 4096;

// The batch kernel's instance for (P, B); !ok(): none.
inline WideKey solve_key(const IpmParams& P, int64_t B) {
    const WideClass c = wide_class(P);
    if (!c.ok) return WideKey{};
    WideKey k{SOLVE, c.model, c.split, P.precision == 1, c.nb, false, 2};
    if (k.f32) {  // (no default-options instance; N <= 64: 3 wavefronts per SIMD, mpcg_wide_kern.h)
        k.wpe = c.nb == 1 ? 3 : 2;
        return k;
    }
    // (default Ipopt options: the instances that compile them as constants -- the benchmark
    // configuration, configs[4]'s bicycle, and every fp64 horizon of the differential drive
    // and the bicycle's 33..64 stages at two wavefronts per SIMD)
    k.defopt = ipopt_options_are_default(P);
    const bool bench = c.model == 0 && c.split && k.defopt;  // (the benchmark configuration)
    if (c.one || (bench && B <= kLoneBatch)) k.wpe = 1;
    // (no default-options instance -- the bicycle at one wavefront per SIMD: the general one)
    if (k.defopt && find_key(k) < 0) k.defopt = false;
    return k;
}
// the resume kernel of a solve kernel's instance (the general-options instance also for the
// default-options one: the two compute bitwise the same); for the fp32 solver the fp64
// instance of the same horizon (a precision-1 launch parks nothing -- the fp32 phase hands every
// ending to the fp64 phase, no_restoration = 1 keeps it -- so its workers find nothing and exit)
inline WideKey resume_key(const IpmParams& P, WideKind kind = RESUME) {
    const WideClass c = wide_class(P);
    return c.ok ? WideKey{kind, c.model, c.split, false, c.nb, false, 0} : WideKey{};
}
// Per-problem parameter rows: the general-options fp64 instance of the horizon class (the rows
// fix neither the class nor the LDS layout: N, the model and filter_cap are P's), or the
// default-options one where the library carries it (the benchmark class); the fp32
// configuration is refused -- its fp64 phase and head would need per-problem instances as well
inline WideKey pp_solve_key(const IpmParams& P, int64_t /*B*/) {
    const WideClass c = wide_class(P);
    if (!c.ok || P.precision != 0) return WideKey{};
    WideKey k{PP_SOLVE, c.model, c.split, false, c.nb, ipopt_options_are_default(P), c.one ? 1 : 2};
    if (k.defopt && find_key(k) < 0) k.defopt = false;
    return k;
}
inline WideKey pp_resume_key(const IpmParams& P) { return P.precision == 0 ? resume_key(P, PP_RESUME) : WideKey{}; }
// A solve started from a record: the general-options fp64 instance of the horizon class (with or
// without parameter rows), its resume kernel by the class as well; the fp32 configuration is
// refused
inline WideKey start_key(const IpmParams& P) {
    const WideClass c = wide_class(P);
    if (!c.ok || P.precision != 0) return WideKey{};
    return WideKey{START, c.model, c.split, false, c.nb, false, c.one ? 1 : 2};
}
inline WideKey start_resume_key(const IpmParams& P) {
    return P.precision == 0 ? resume_key(P, START_RESUME) : WideKey{};
}
// the resume instance that continues what a batch kernel of kind `batch` parks or lists
inline WideKey resume_key_of(int batch, const IpmParams& P) {
    return batch == PP_SOLVE ? pp_resume_key(P) : batch == START ? start_resume_key(P) : resume_key(P);
}
// the fp64 phase's instance (k_warm_wide, default options) for the horizon class of the fp64
// parameters Pr (fp64_params): the differential drive only
inline WideKey warm_key(const IpmParams& Pr) {
    const WideClass c = wide_class(Pr);
    return c.ok && Pr.model == 0 ? WideKey{WARM, 0, c.split, false, c.nb, true, c.one ? 1 : 2} : WideKey{};
}

// ---------------------------------------------------------------- the two-phase configuration
// The fp32 configuration (mpcg_params.precision 1) runs in two phases: the fp32 solver on the
// whole batch (its stated options), then the fp64 solver with the reference's Ipopt options on
// the whole batch again (k_warm_wide) -- from the fp32 solver's converged iterate (a few fp64
// iterations to Ipopt's tolerance), or from the start where the fp32 solve did not converge
// (its line search fails where Ipopt would enter the restoration phase, a tiny step, the
// iteration limit: a float iterate's noise floor).  mpcg_params.no_restoration = 1 keeps the
// fp32 solver's own ending instead (status 9 where Ipopt would restore).
inline bool two_phase(const IpmParams& P) { return P.precision == 1 && !P.no_resto; }
inline IpmParams fp64_params(const IpmParams& P) {
    IpmParams q = P;
    q.precision = 0;
    ipopt_default_options(q);
    return q;
}
// The fp32 configuration's head: the problems the solve order ranks longest (ordered batches only,
// B / 1024 of them) are solved by the fp64 solver from the start on the aux stream while the fp32
// phase runs the others -- the longest fp64 solves (through the restoration phase) would otherwise
// start only with the fp64 phase and set its length (problem 19,304 of the infinity set at N = 40:
// rank 2 of the order, 217 fp64 iterations, 11.5 ms alone).
inline int64_t head_count(int64_t B) {
    int64_t div = 1024;
#ifdef MPCG_HEAD_ENV
    // (diagnostic builds only: the head's share of the batch, B / MPCG_HEAD_DIV; 0: no head)
    if (const char* d = getenv("MPCG_HEAD_DIV")) div = atol(d);
    if (div <= 0) return 0;
#endif
    return B > kOrderMinBatch ? B / div : 0;
}
// the head's parameters: the fp64 solver's, with a park entry for every head problem (no
// park-area overflow: the head's stream never waits for its resume workers' stream)
inline IpmParams head_params(const IpmParams& P, int64_t K) {
    IpmParams q = fp64_params(P);
    q.park_cap = (int)K;
    return q;
}

// ---------------------------------------------------------------- the workspace
constexpr size_t kWsAlign = 256, kLine = 128;  // regions; slots and park entries: whole lines

// Workspace slots for a batch of B: the slot budget -- four times the wavefronts the device can
// hold resident at once, mpcg_wide.hip slot_budget -- at most B (at least 32 per XCD), in one
// equal partition per XCD.  A wavefront claims slot blockIdx mod the partition size in its
// XCD's partition, or the next free one: with the margin, a slow problem still holding a slot
// rarely makes a later wavefront probe further.
inline int64_t slot_count(int64_t budget, int64_t B, int nxcc) {
    if (B <= 0) return 0;
    const int64_t n = budget < B ? budget : B, floor_ = B < 32 ? B : 32;
    const int64_t part = (n + nxcc - 1) / nxcc;
    return (part > floor_ ? part : floor_) * nxcc;
}
// the park area: problems that enter the restoration phase (rare: ~5e-5 of the infinity set at
// N = 20, 5e-4 at N = 40, ~4e-3 with the fp32 solver at N = 40); its capacity is B / 128, at
// least 256 (P.park_cap > 0: that many, mpcg_set_park_capacity).  Beyond it a problem goes to
// the overflow list and is solved again from the start after the drain.
inline int64_t wide_park_cap(const IpmParams& P, int64_t B) {
    int64_t c = B / 128 > 256 ? B / 128 : 256;
    if (P.park_cap > 0) c = P.park_cap;
    return c < B ? c : B;
}

struct Region {
    size_t off = 0, bytes = 0;  // (bytes: what the region reserves)
    size_t end() const { return off + bytes; }
};
// One phase's workspace: slot flags | counters | park indices | park ready flags | overflow list
// | slots | park area.  Offsets from the phase's base.
struct PhaseLayout {
    // the 64 counters (int32_t, one 256-byte block)
    enum Counter { PARK_COUNT, PARK_TAKEN, DONE, STARTED, OVF_COUNT, OVF_TAKEN, N_COUNTERS = 64 };
    int64_t B = 0, nslots = 0, park_cap = 0;
    int nxcc = 0;
    size_t elem = 0;         // bytes of the solver's arithmetic type
    int64_t slot_elems = 0;  // a slot: WideLayout::spill() in whole 128-byte lines
    int64_t park_stride = 0;  // a park entry: WideLayout::park() in whole 128-byte lines
    Region flags, counters, park_idx, park_ready, ovf, slots, park;
    size_t total = 0;
    // the overflow list: one index per problem (only where the park area can overflow)
    bool has_ovf() const { return park_cap < B; }

    PhaseLayout() = default;
    PhaseLayout(const IpmParams& P, int64_t B_, int64_t budget, int nxcc_)
        : B(B_), nslots(slot_count(budget, B_, nxcc_)), park_cap(wide_park_cap(P, B_)), nxcc(nxcc_), elem(elem_bytes(P)) {
        const WideLayout L(P.N, P.filter_cap, P.model);
        slot_elems = (int64_t)round_up((size_t)L.spill(), kLine / elem);
        park_stride = (int64_t)round_up((size_t)L.park(), kLine / elem);
        auto take = [this](size_t bytes) {
            const Region r{total, bytes};
            total += bytes;
            return r;
        };
        flags = take(round_up((size_t)nslots * sizeof(int32_t), kWsAlign));
        counters = take(N_COUNTERS * sizeof(int32_t));
        park_idx = take(round_up((size_t)park_cap * sizeof(int64_t), kWsAlign));
        park_ready = take(round_up((size_t)park_cap * sizeof(int32_t), kWsAlign));
        ovf = take(has_ovf() ? round_up((size_t)B * sizeof(int64_t), kWsAlign) : 0);
        slots = take((size_t)slot_elems * elem * (size_t)nslots);
        park = take((size_t)park_stride * elem * (size_t)park_cap);
    }
};

// A handle's whole workspace.  One phase at offset 0; the fp32 configuration: the larger of its
// two phases' workspaces (the phases run one after the other), then the hand-over
// (handoff_stride floats per problem: WideLayout::handoff in whole lines), the fp64 phase's
// solve order (B indices, then its two counters -- k_cold_first), and the head's workspace.
// budget(P, B): the slot budget of a phase, asked once per phase.
struct SolveLayout {
    bool two = false;
    PhaseLayout first, second;  // second: the fp64 phase (the fp32 configuration)
    size_t phases = 0;          // bytes at offset 0 that the phases share
    Region handoff, order2, cnt2;
    int64_t handoff_stride = 0;
    int64_t head_n = 0;  // problems of the head the workspace has room for (head_count)
    size_t head_off = 0;
    PhaseLayout head;
    size_t total = 0;

    template <class Budget>
    SolveLayout(const IpmParams& P, int64_t B, int nxcc, Budget&& budget)
        : two(two_phase(P)), first(P, B, budget(P, B), nxcc), phases(first.total), total(first.total) {
        if (!two) return;
        const IpmParams Pr = fp64_params(P);
        second = PhaseLayout(Pr, B, budget(Pr, B), nxcc);
        phases = first.total > second.total ? first.total : second.total;
        handoff_stride = (int64_t)round_up((size_t)WideLayout::handoff(P.N), kLine / sizeof(float));
        handoff = Region{round_up(phases, kWsAlign), (size_t)handoff_stride * sizeof(float) * (size_t)B};
        order2 = Region{handoff.end(), round_up((size_t)B, 64) * sizeof(int32_t)};
        cnt2 = Region{order2.end(), 64 * sizeof(int32_t)};
        head_off = total = round_up(cnt2.end(), kWsAlign);
        head_n = head_count(B);
        if (head_n > 0) {
            const IpmParams Ph = head_params(P, head_n);
            head = PhaseLayout(Ph, head_n, budget(Ph, head_n), nxcc);
            total = head_off + head.total;
        }
    }
};

// ---------------------------------------------------------------- the tick scratch
// The intermediates of one control tick of B robots (mpcg_api.cpp tick), one handle buffer:
// state [B][6] | coeffs [B][4] | u0 [B][2] | the robots' parameter rows [B][16] (rows != 0: the
// tick with a goal, the rollout) | and for the rollout (Mmax > 0: its plan rows per robot) cmd
// [B][3] | the windows' plans [B][Mmax][2] | count [B] | start [B].  Doubles first, the two int32
// regions last; every region from an 8-byte boundary.  The warm tick (warm != 0: the rollout
// started from the carried records, mpcg_rollout_device_start) appends mu0 [B] | mode [B] | a status
// scratch [B] (where the caller logs no status); without it the layout is byte for byte the
// three-argument one.  Nothing in it outlives a call, so the layout may differ from one call to
// the next.
constexpr int kRowFields = 16;  // (MPCG_PP_FIELDS of include/mpcg.h, which this header does not need)
struct TickLayout {
    Region state, coeffs, u0, rows, cmd, plan, count, start, mu0, mode, status;
    size_t total = 0;
    TickLayout(int64_t B, int Mmax, int rows_, int warm = 0) {
        const size_t b = (size_t)B, roll = Mmax > 0 ? b : 0, wm = warm ? b : 0;
        auto take = [this](size_t bytes) {
            const Region r{total, round_up(bytes, 8)};
            total += r.bytes;
            return r;
        };
        state = take(sizeof(double) * 6 * b);
        coeffs = take(sizeof(double) * 4 * b);
        u0 = take(sizeof(double) * 2 * b);
        rows = take(rows_ ? sizeof(double) * kRowFields * b : 0);
        cmd = take(sizeof(double) * 3 * roll);
        plan = take(sizeof(double) * 2 * (size_t)Mmax * roll);
        count = take(sizeof(int32_t) * roll);
        start = take(sizeof(int32_t) * roll);
        mu0 = take(sizeof(double) * wm);
        mode = take(sizeof(int32_t) * wm);
        status = take(sizeof(int32_t) * wm);
    }
};

// ---------------------------------------------------------------- the host solve's staging
// The device copies of a host solve's arrays (mpcg_api.cpp solve_host), one handle buffer: state
// [B][6] | coeffs [B][4] | u0 [B][2] | traj [B][3][N] | obj [B] | mu0 [B] (a start) | the records
// [B][solution_elems(N)] (a start, the solution out, or both: solved in place) | the parameter rows
// [B][16] (rows) | then int32: status [B] | iters [B] | diag [B][4] | mode [B] | used [B] (a start).
// Every region from an 8-byte boundary, as TickLayout's.
struct IoLayout {
    Region state, coeffs, u0, traj, obj, mu0, rec, rows, status, iters, diag, mode, used;
    size_t total = 0;
    IoLayout(int64_t B, int N, bool rows_, bool sol, bool start) {
        const size_t b = (size_t)B, st = start ? b : 0;
        auto take = [this](size_t bytes) {
            const Region r{total, round_up(bytes, 8)};
            total += r.bytes;
            return r;
        };
        state = take(sizeof(double) * 6 * b);
        coeffs = take(sizeof(double) * 4 * b);
        u0 = take(sizeof(double) * 2 * b);
        traj = take(sizeof(double) * 3 * (size_t)N * b);
        obj = take(sizeof(double) * b);
        mu0 = take(sizeof(double) * st);
        rec = take(sol || start ? sizeof(double) * (size_t)solution_elems(N) * b : 0);
        rows = take(rows_ ? sizeof(double) * kRowFields * b : 0);
        status = take(sizeof(int32_t) * b);
        iters = take(sizeof(int32_t) * b);
        diag = take(sizeof(int32_t) * 4 * b);
        mode = take(sizeof(int32_t) * st);
        used = take(sizeof(int32_t) * st);
    }
};

}  // namespace mpcg
#endif
