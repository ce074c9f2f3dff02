// tests/native/wide_plan_check.cpp -- the launch plan of the wavefront solver
// (mpc_ros_amd/csrc/wide_plan.h: the choice among the instances of every kind, workspace layout,
// tick scratch layout, the host solve's staging layout) on the host; no GPU runtime.  Checks the
// properties below (exit status 1 and a message at the first that fails), and prints the chosen
// solve instance over the whole input space as JSON, run-length encoded over the horizon:
// {"model<m>_precision<p>_<default|option>_B<B>": [[N from, N to, name], ...]} ("": refused) --
// tests/test_host_logic.py compares it with tests/golden/launch_plan.json.  With the argument
// "pp" it prints the per-problem solve instance chosen under a non-default option per (model,
// horizon range) instead (tests/test_pparams_host.py).
//
//   g++ -std=c++20 -o wide_plan_check tests/native/wide_plan_check.cpp && ./wide_plan_check [pp]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../mpc_ros_amd/csrc/wide_plan.h"

using namespace mpcg;

#define CHECK(c, ...)                                      \
    do {                                                   \
        if (!(c)) {                                        \
            std::fprintf(stderr, "FAILED: %s -- ", #c);    \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

static IpmParams params(int N, int model, int precision, bool option) {
    IpmParams P{};
    ipopt_default_options(P);
    P.N = N;
    P.model = model;
    P.precision = precision;
    P.lf = 0.5;
    if (option) P.tol = 1e-7;  // (one non-default option)
    return P;
}

// ------------------------------------------------------------------ the instance list
static bool g_used[kWideInstances];
// a chosen key is a row of the list under its kind; the row's index
static int use(const WideKey& k, int kind, const char* fn, int model, int prec, int N, int opt, long B) {
    CHECK(k.ok(), "%s refuses model %d precision %d N %d option %d B %ld", fn, model, prec, N, opt, B);
    const int i = find_key(k);
    CHECK(k.kind == kind && i >= 0 && kWideKeys[i].kind == kind,
          "%s of model %d precision %d N %d option %d B %ld is not in the list under its kind", fn, model, prec, N,
          opt, B);
    g_used[i] = true;
    return i;
}
static bool same_but_kind(WideKey a, const WideKey& b) {
    a.kind = b.kind;
    return a == b;
}

// Every key function over model x precision x N = 1..128 x default / non-default options x
// B in {1, 4096, 4097}.  pp_table: prints the per-problem solve instance chosen under a
// non-default option per (model, horizon range) instead of the solve instances' JSON.
static void check_instances(bool pp_table) {
    static_assert(sizeof(kWideNames) / sizeof(kWideNames[0]) == kWideInstances &&
                  sizeof(kWideGroupOf) / sizeof(kWideGroupOf[0]) == kWideInstances);
    if (!pp_table) std::printf("{\n");
    bool first = true;
    for (int model = 0; model < 2; ++model)
        for (int prec = 0; prec < 2; ++prec)
            for (int opt = 0; opt < 2; ++opt)
                for (long B : {1L, 4096L, 4097L}) {
                    if (!pp_table)
                        std::printf("%s  \"model%d_precision%d_%s_B%ld\": [", first ? "" : ",\n", model, prec,
                                    opt ? "option" : "default", B);
                    first = false;
                    std::string cur, cur_pp;
                    int from = 1, from_pp = 1;
                    bool f2 = true;
                    for (int N = 1; N <= 129; ++N) {
                        std::string name = "END", name_pp = "END";
                        if (N <= 128) {
                            const IpmParams P = params(N, model, prec, opt);
                            const WideKey k = solve_key(P, B);
                            const bool refused = prec == 1 && model == 1;  // (fp32: the differential drive)
                            CHECK(k.ok() == !refused, "model %d precision %d N %d", model, prec, N);
                            CHECK(resume_key(P).ok() == !refused, "resume: model %d precision %d N %d", model, prec, N);
                            name = "";
                            if (k.ok()) {
                                name = kWideNames[use(k, SOLVE, "solve_key", model, prec, N, opt, B)];
                                use(resume_key(P), RESUME, "resume_key", model, prec, N, opt, B);
                                if (prec == 1)
                                    use(warm_key(fp64_params(P)), WARM, "warm_key", model, prec, N, opt, B);
                            }
                            // rows and a start: fp32 is refused
                            const WideKey pk = pp_solve_key(P, B), prk = pp_resume_key(P);
                            const WideKey sk = start_key(P), srk = start_resume_key(P);
                            CHECK(pk.ok() == (prec == 0) && prk.ok() == (prec == 0), "rows: model %d precision %d N %d",
                                  model, prec, N);
                            CHECK(sk.ok() == (prec == 0) && srk.ok() == (prec == 0), "start: model %d precision %d N %d",
                                  model, prec, N);
                            if (prec == 0) {
                                // fp64, the class and register allocation of the plain general instance
                                // (the key solve_key gives a non-default option at B = 4097); the
                                // per-problem default-options instance only under default options
                                const WideKey plain = solve_key(params(N, model, 0, true), 4097);
                                CHECK(!plain.f32 && !plain.defopt, "model %d N %d: the plain general instance", model, N);
                                const int i = use(pk, PP_SOLVE, "pp_solve_key", model, prec, N, opt, B);
                                CHECK(!pk.f32 && pk.model == plain.model && pk.split == plain.split && pk.nb == plain.nb &&
                                          pk.wpe == plain.wpe && (!pk.defopt || !opt),
                                      "model %d N %d: rows, not the plain general instance's class", model, N);
                                use(prk, PP_RESUME, "pp_resume_key", model, prec, N, opt, B);
                                CHECK(same_but_kind(prk, resume_key(P)), "per-problem resume key of model %d N %d", model, N);
                                use(sk, START, "start_key", model, prec, N, opt, B);
                                CHECK(same_but_kind(sk, plain), "model %d N %d: start, not the plain general instance", model,
                                      N);
                                use(srk, START_RESUME, "start_resume_key", model, prec, N, opt, B);
                                CHECK(same_but_kind(srk, resume_key(P)), "started resume key of model %d N %d", model, N);
                                name_pp = kWideNames[i];
                            }
                        }
                        if (N == 1) cur = name, cur_pp = name_pp;
                        if (name != cur) {
                            if (!pp_table) std::printf("%s[%d, %d, \"%s\"]", f2 ? "" : ", ", from, N - 1, cur.c_str());
                            f2 = false;
                            cur = name;
                            from = N;
                        }
                        if (name_pp != cur_pp) {
                            if (pp_table && prec == 0 && opt == 1 && B == 4097)
                                std::printf("model %d N %d..%d %s\n", model, from_pp, N - 1, cur_pp.c_str());
                            cur_pp = name_pp;
                            from_pp = N;
                        }
                    }
                    if (!pp_table) std::printf("]");
                }
    if (!pp_table) std::printf("\n}\n");
    // no dead instance
    for (int i = 0; i < kWideInstances; ++i) CHECK(g_used[i], "instance %s is never chosen", kWideNames[i]);
    // refusals: more than 128 stages
    const IpmParams P129 = params(129, 0, 0, false);
    CHECK(!solve_key(P129, 1).ok() && !resume_key(P129).ok() && !warm_key(P129).ok() && !pp_solve_key(P129, 1).ok() &&
              !pp_resume_key(P129).ok() && !start_key(P129).ok() && !start_resume_key(P129).ok(),
          "N = 129");
    // the groups: 0 .. kWideGroups - 1, none empty
    bool seen[kWideGroups] = {};
    for (int g : kWideGroupOf) {
        CHECK(g >= 0 && g < kWideGroups, "group %d", g);
        seen[g] = true;
    }
    for (int g = 0; g < kWideGroups; ++g) CHECK(seen[g], "group %d has no instance", g);
}

// ------------------------------------------------------------------ the workspace layout
static void check_phase(const PhaseLayout& W, const IpmParams& P, int64_t B, int64_t budget, int nxcc, const char* what) {
    const WideLayout L(P.N, P.filter_cap, P.model);
    const size_t eb = P.precision == 1 ? 4 : 8;
    CHECK(W.B == B && W.nxcc == nxcc && W.elem == eb, "%s", what);
    // slots: equal partitions per XCD, at least min(B, 32) each, at least min(budget, B) in all
    CHECK(W.nslots % nxcc == 0 && W.nslots / nxcc >= (B < 32 ? B : 32) && W.nslots >= (budget < B ? budget : B) &&
              W.nslots < (budget < B ? budget : B) + (B < 32 ? B : 32) * nxcc + nxcc,
          "%s: nslots %lld", what, (long long)W.nslots);
    const int64_t cap = P.park_cap > 0 ? P.park_cap : (B / 128 > 256 ? B / 128 : 256);
    CHECK(W.park_cap == (cap < B ? cap : B), "%s: park_cap %lld", what, (long long)W.park_cap);
    // whole 128-byte lines that hold the solver's own counts
    CHECK(W.slot_elems >= L.spill() && (size_t)W.slot_elems * eb % 128 == 0 &&
              (size_t)(W.slot_elems - L.spill()) * eb < 128,
          "%s: slot_elems", what);
    CHECK(W.park_stride >= L.park() && (size_t)W.park_stride * eb % 128 == 0 &&
              (size_t)(W.park_stride - L.park()) * eb < 128,
          "%s: park_stride", what);
    // the regions in the stated order, each from a 256-byte boundary, none overlapping the next
    const Region* r[] = {&W.flags, &W.counters, &W.park_idx, &W.park_ready, &W.ovf, &W.slots, &W.park};
    CHECK(r[0]->off == 0, "%s", what);
    for (int i = 0; i < 7; ++i) {
        CHECK(r[i]->off % 256 == 0, "%s: region %d at %zu", what, i, r[i]->off);
        if (i > 0) CHECK(r[i]->off == r[i - 1]->end(), "%s: region %d", what, i);
    }
    CHECK(W.total == W.park.end(), "%s: total", what);
    // each holds what it is for
    CHECK(W.flags.bytes >= (size_t)W.nslots * 4, "%s: flags", what);
    CHECK(W.counters.bytes == 64 * 4 && PhaseLayout::OVF_TAKEN < PhaseLayout::N_COUNTERS, "%s: counters", what);
    CHECK(W.park_idx.bytes >= (size_t)W.park_cap * 8 && W.park_ready.bytes >= (size_t)W.park_cap * 4, "%s: park flags", what);
    CHECK(W.has_ovf() == (W.park_cap < B) && (W.ovf.bytes > 0) == W.has_ovf() &&
              (!W.has_ovf() || W.ovf.bytes >= (size_t)B * 8),
          "%s: overflow list", what);
    CHECK(W.slots.bytes == (size_t)W.nslots * W.slot_elems * eb, "%s: slots", what);
    CHECK(W.park.bytes == (size_t)W.park_cap * W.park_stride * eb, "%s: park area", what);
}

static int check_layouts() {
    int cases = 0;
    for (int N : {1, 20, 32, 33, 64, 65, 128})
        for (int model : {0, 1})
            for (int prec : {0, 1, 2})  // (2: fp32 with no_resto)
                for (int64_t B : {1, 2, 31, 33, 2048, 2049, 65536})
                    for (int64_t pcap : {(int64_t)0, (int64_t)1, B})
                        for (int v : {0, 1}) {
                            // (the fallback budget on 8 XCDs; a count that 4 XCDs do not divide)
                            const int64_t budget = v == 0 ? 4096 : 1003;
                            const int nxcc = v == 0 ? 8 : 4;
                            IpmParams P = params(N, model, prec ? 1 : 0, false);
                            P.no_resto = prec == 2;
                            P.park_cap = (int)pcap;
                            int asked = 0;
                            const SolveLayout W(P, B, nxcc, [&](const IpmParams&, int64_t) {
                                ++asked;
                                return budget;
                            });
                            char what[128];
                            std::snprintf(what, sizeof what, "N %d model %d precision %d B %lld park_cap %lld nxcc %d", N,
                                          model, prec, (long long)B, (long long)pcap, nxcc);
                            ++cases;
                            check_phase(W.first, P, B, budget, nxcc, what);
                            if (prec != 1) {  // one phase at offset 0
                                CHECK(!W.two && W.total == W.first.total && W.head_n == 0 && asked == 1, "%s", what);
                                continue;
                            }
                            const IpmParams Pr = fp64_params(P);
                            check_phase(W.second, Pr, B, budget, nxcc, what);
                            CHECK(W.two && W.phases == (W.first.total > W.second.total ? W.first.total : W.second.total),
                                  "%s: phases", what);
                            // the hand-over after the phases, whole lines that hold the solver's count
                            CHECK(W.handoff.off % 256 == 0 && W.handoff.off >= W.phases, "%s: hand-over", what);
                            CHECK(W.handoff_stride >= WideLayout::handoff(N) && W.handoff_stride % 32 == 0 &&
                                      W.handoff_stride - WideLayout::handoff(N) < 32 &&
                                      W.handoff.bytes == (size_t)W.handoff_stride * 4 * (size_t)B,
                                  "%s: hand-over stride", what);
                            // the fp64 phase's order, then its two counters in the space reserved for them
                            CHECK(W.order2.off == W.handoff.end() && W.order2.off % 4 == 0 &&
                                      W.order2.bytes >= (size_t)B * 4,
                                  "%s: order", what);
                            CHECK(W.cnt2.off == W.order2.end() && W.cnt2.bytes >= 2 * 4 && W.cnt2.end() <= W.head_off,
                                  "%s: order counters", what);
                            CHECK(W.head_off % 256 == 0, "%s: head offset", what);
                            // the head: exactly beyond 2048 problems (ordered batches)
                            CHECK((W.head_n > 0) == (B > 2048) && (W.head.total > 0) == (B > 2048) &&
                                      W.total == W.head_off + W.head.total && asked == (B > 2048 ? 3 : 2),
                                  "%s: head", what);
                            if (W.head_n > 0) {
                                CHECK(W.head_n == B / 1024, "%s: head count", what);
                                const IpmParams Ph = head_params(P, W.head_n);
                                check_phase(W.head, Ph, W.head_n, budget, nxcc, what);
                                CHECK(!W.head.has_ovf(), "%s: a park entry per head problem", what);
                                // (the phases beside a head cover B - K problems, in the space reserved for B)
                                const int64_t Bm = B - W.head_n;
                                CHECK(PhaseLayout(P, Bm, budget, nxcc).total <= W.phases &&
                                          PhaseLayout(Pr, Bm, budget, nxcc).total <= W.phases,
                                      "%s: the phases beside the head", what);
                            }
                        }
    return cases;
}

// ------------------------------------------------------------------ the tick scratch
static int check_tick_layouts() {
    int cases = 0;
    for (int64_t B : {1, 63, 64, 65, 4097})
        for (int Mmax : {0, 2, 11, 64})
            for (int rows : {0, 1}) {
                const TickLayout L(B, Mmax, rows);
                char what[64];
                std::snprintf(what, sizeof what, "tick B %lld Mmax %d rows %d", (long long)B, Mmax, rows);
                ++cases;
                // the regions in the stated order, each from an 8-byte boundary, none overlapping the
                // next; the int32 regions last; the total is the end of the last one
                const Region* r[] = {&L.state, &L.coeffs, &L.u0, &L.rows, &L.cmd, &L.plan, &L.count, &L.start};
                CHECK(r[0]->off == 0, "%s", what);
                for (int i = 0; i < 8; ++i) {
                    CHECK(r[i]->off % 8 == 0, "%s: region %d at %zu", what, i, r[i]->off);
                    if (i > 0) CHECK(r[i]->off == r[i - 1]->end(), "%s: region %d", what, i);
                }
                CHECK(L.total == L.start.end(), "%s: total", what);
                // each holds what it is for
                const size_t b = (size_t)B, roll = Mmax > 0 ? b : 0;
                CHECK(L.state.bytes == 48 * b && L.coeffs.bytes == 32 * b && L.u0.bytes == 16 * b, "%s: the solve's", what);
                CHECK(L.rows.bytes == (rows ? 8 * 16 * b : 0), "%s: rows", what);
                CHECK(L.cmd.bytes == 24 * roll && L.plan.bytes == 16 * (size_t)Mmax * roll, "%s: cmd, plan", what);
                CHECK(L.count.bytes >= 4 * roll && L.start.bytes >= 4 * roll, "%s: count, start", what);
                // the plain tick: 12 B doubles; in all what the three buffers it replaces took (12 B,
                // 16 B and (2 Mmax + 3) B doubles + 2 B int32), but for the two int32 regions'
                // padding to whole doubles (an odd B)
                if (!rows && !Mmax) CHECK(L.total == 96 * b, "%s: the plain tick", what);
                const size_t before = 96 * b + (rows ? 128 * b : 0) + (8 * (2 * (size_t)Mmax + 3) + 8) * roll;
                CHECK(L.total == before + (B % 2 ? 8 * roll / b : 0), "%s: footprint %zu, was %zu", what, L.total, before);
            }
    return cases;
}

// ------------------------------------------------------------------ the host solve's staging
static int check_io_layouts() {
    int cases = 0;
    for (int64_t B : {1, 3, 4096})
        for (int N : {2, 20, 128})
            for (int rows : {0, 1})
                for (int sol : {0, 1})
                    for (int start : {0, 1}) {
                        const IoLayout L(B, N, rows, sol, start);
                        char what[80];
                        std::snprintf(what, sizeof what, "io B %lld N %d rows %d sol %d start %d", (long long)B, N, rows,
                                      sol, start);
                        ++cases;
                        // the regions in the stated order, each from an 8-byte boundary, none
                        // overlapping the next; the int32 regions last; the total is the end of the last
                        const Region* r[] = {&L.state, &L.coeffs, &L.u0,    &L.traj, &L.obj,  &L.mu0, &L.rec,
                                             &L.rows,  &L.status, &L.iters, &L.diag, &L.mode, &L.used};
                        CHECK(r[0]->off == 0, "%s", what);
                        for (int i = 0; i < 13; ++i) {
                            CHECK(r[i]->off % 8 == 0, "%s: region %d at %zu", what, i, r[i]->off);
                            if (i > 0) CHECK(r[i]->off == r[i - 1]->end(), "%s: region %d", what, i);
                        }
                        CHECK(L.total == L.used.end(), "%s: total", what);
                        // each holds what it is for
                        const size_t b = (size_t)B, st = start ? b : 0, ne = (size_t)solution_elems(N);
                        CHECK(L.state.bytes == 48 * b && L.coeffs.bytes == 32 * b && L.u0.bytes == 16 * b &&
                                  L.traj.bytes == 24 * (size_t)N * b && L.obj.bytes == 8 * b,
                              "%s: the solve's", what);
                        CHECK(L.mu0.bytes == 8 * st && L.rec.bytes == (sol || start ? 8 * ne * b : 0) &&
                                  L.rows.bytes == (rows ? 8 * 16 * b : 0),
                              "%s: mu0, records, rows", what);
                        CHECK(L.status.bytes >= 4 * b && L.status.bytes < 4 * b + 8 && L.iters.bytes >= 4 * b &&
                                  L.iters.bytes < 4 * b + 8 && L.diag.bytes == 16 * b,
                              "%s: status, iters, diag", what);
                        CHECK(L.mode.bytes >= 4 * st && L.mode.bytes < 4 * st + 8 && L.used.bytes >= 4 * st &&
                                  L.used.bytes < 4 * st + 8,
                              "%s: mode, used", what);
                    }
    return cases;
}

// (argument "pp": the per-problem table on the standard output instead of the JSON)
int main(int argc, char** argv) {
    check_instances(argc > 1 && std::string(argv[1]) == "pp");
    const int cases = check_layouts() + check_tick_layouts() + check_io_layouts();
    std::fprintf(stderr, "wide_plan_check: %d layouts ok\n", cases);
    return 0;
}
