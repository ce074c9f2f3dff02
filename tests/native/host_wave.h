// tests/native/host_wave.h -- TEST HARNESS ONLY.
//
// The host emulation of the one-problem-per-wavefront solver (mpc_ros_amd/csrc/wide_core.h), once,
// for the wide_*_check programs: the 64 lanes of a wavefront are 64 cooperative fibers (ucontext)
// on one thread, LDS is a shared array, a lane exchange is a store / barrier / load / barrier, and
// the wave barrier passes control round-robin to the next lane (lane 0 resumes once lane 63 has
// arrived: every lane calls the same barriers, as on the device).  The butterflies run the same
// pairwise operations as the device shuffles.  Problems run in parallel, one OS thread each
// (MPCG_HOST_THREADS, default the machine's CPUs).  The fibers are the only lane model: the mode
// that ran the lanes as 64 OS threads on a std::barrier was built by nothing and is gone.
// Never part of the product library.
//
// Besides the wavefront (Fibers, HostShared, HostWave; HOST_T / HT: -DHOST_T=float is the fp32
// solver) it holds what every program needs around it:
//   read_params, read_problems   the shared head of stdin (below)
//   Scratch                      a problem's LDS image, workspace slot and park entry, NaN-filled
//   with_solver                  the WideSolver instance of a (model, N), handed to a callable
//   continue_parked              the resume kernel's part: park, entry check, unpark, finish_resto
//   run_problems                 the worker pool; the output lines in problem order
//   append, append_values, append_image   the output formats
//
// stdin:  N dt ref_cte ref_eth ref_v w_cte w_eth w_v w_w w_a w_dw w_da max_w max_a bound tol max_iter
//         model lf
//         the Ipopt options, one "name value" line each under Ipopt's name (the third column of
//         ipm_core.h's MPCG_IPOPT_OPTIONS) or cpu_iter_budget, in any order, closed by a line
//         "end": an option left out keeps Ipopt's default (no iteration budget), an unknown
//         name ends the run with exit status 2
//         B, then B x (state[6], coeffs[4])
//         (malformed or truncated input: exit status 1)
#pragma once
#include <atomic>
#include <cinttypes>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <ucontext.h>
#ifdef __SANITIZE_ADDRESS__
#include <sanitizer/common_interface_defs.h>
#endif

#include "../../mpc_ros_amd/csrc/wide_core.h"

// 64 lanes as fibers on the calling thread: wait() hands control to the next lane in
// round-robin order, so a lane resumes after every other lane has reached the same barrier
struct Fibers {
    static constexpr size_t kStack = 4u << 20;  // (lazily committed)
    ucontext_t main_ctx, ctx[64];
    std::unique_ptr<char[]> stack[64];
    int ndone = 0;
    void* fn = nullptr;  // the lane body: void(int lane)
    void (*call)(void*, int) = nullptr;
#ifdef __SANITIZE_ADDRESS__
    void* fake = nullptr;
#endif
    void swap_to(ucontext_t* from, int to_lane) {
#ifdef __SANITIZE_ADDRESS__
        __sanitizer_start_switch_fiber(&fake, stack[to_lane].get(), kStack);
#endif
        swapcontext(from, &ctx[to_lane]);
#ifdef __SANITIZE_ADDRESS__
        __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
    }
    void wait(int t) { swap_to(&ctx[t], (t + 1) & 63); }
    static void entry(int hi, int lo, int t) {
        Fibers* f = (Fibers*)(((uintptr_t)(unsigned)hi << 32) | (uintptr_t)(unsigned)lo);
#ifdef __SANITIZE_ADDRESS__
        __sanitizer_finish_switch_fiber(f->fake, nullptr, nullptr);
#endif
        f->call(f->fn, t);
        // a finished lane passes on; the last one returns to the caller
        if (++f->ndone == 64) {
#ifdef __SANITIZE_ADDRESS__
            __sanitizer_start_switch_fiber(nullptr, nullptr, 0);
#endif
            setcontext(&f->main_ctx);
        }
        f->swap_to(&f->ctx[t], (t + 1) & 63);
    }
    template <class F>
    void run(F& body) {
        fn = &body;
        call = [](void* b, int t) { (*(F*)b)(t); };
        const uintptr_t me = (uintptr_t)this;
        for (int t = 0; t < 64; ++t) {
            if (!stack[t]) stack[t].reset(new char[kStack]);
            getcontext(&ctx[t]);
            ctx[t].uc_stack.ss_sp = stack[t].get();
            ctx[t].uc_stack.ss_size = kStack;
            ctx[t].uc_link = nullptr;
            makecontext(&ctx[t], (void (*)())entry, 3, (int)(me >> 32), (int)(me & 0xffffffffu), t);
        }
        ndone = 0;
#ifdef __SANITIZE_ADDRESS__
        __sanitizer_start_switch_fiber(&fake, stack[0].get(), kStack);
#endif
        swapcontext(&main_ctx, &ctx[0]);
#ifdef __SANITIZE_ADDRESS__
        __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
    }
};

struct HostShared {
    Fibers* fib = nullptr;
    double xd[64];
    int xi[64];
    std::vector<double> lds;
};

#ifndef HOST_T
#define HOST_T double  // -DHOST_T=float: the fp32 solver
#endif
typedef HOST_T HT;

struct HostWave {
    HostShared* sh;
    int t;
    double* lds;
    double* S() const { return lds; }
    template <class U>
    U* Sp() const { return reinterpret_cast<U*>(lds); }
    void sync() const { sh->fib->wait(t); }
    void gsync() const { sync(); }
    template <class U>
    U from(U v, int src) const {
        sh->xd[t] = (double)v;
        sync();
        const U r = (U)sh->xd[src];
        sync();
        return r;
    }
    double xor_(double v, int m) const {
        sh->xd[t] = v;
        sync();
        const double r = sh->xd[t ^ m];
        sync();
        return r;
    }
    template <class U>
    U up1(U v) const {
        sh->xd[t] = (double)v;
        sync();
        const U r = t > 0 ? (U)sh->xd[t - 1] : v;
        sync();
        return r;
    }
    bool any(bool b) const {
        sh->xi[t] = b ? 1 : 0;
        sync();
        int r = 0;
        for (int i = 0; i < 64; ++i) r |= sh->xi[i];
        sync();
        return r != 0;
    }
    int uni(int v) const { return v; }
    int ballot_prefix(bool b, int* total) const {
        sh->xi[t] = b ? 1 : 0;
        sync();
        int c = 0, n = 0;
        for (int i = 0; i < 64; ++i) {
            n += sh->xi[i];
            if (i < t) c += sh->xi[i];
        }
        sync();
        *total = n;
        return c;
    }
    int lane() const { return t; }
    void mark(int) const {}
    void sched_fence() const {}
    template <class U>
    void ld2(int i, U& a, U& b) const {
        if (i & 1) {  // (the device's pair load is a 16-byte (fp32: 8-byte) aligned access)
            std::fprintf(stderr, "ld2 at odd index %d\n", i);
            std::abort();
        }
        a = Sp<U>()[i];
        b = Sp<U>()[i + 1];
    }
    template <class U>
    U dn1(U v) const { return from(v, t < 63 ? t + 1 : t); }
    // device: DPP wave_shr:1 / wave_shl:1 with bound_ctrl off (lane 0 / 63 keeps x)
    template <class U>
    void up8(U* x, const U* y) const {
        for (int q = 0; q < 8; ++q) {
            const U r = from(y[q], t > 0 ? t - 1 : t);
            if (t > 0) x[q] = r;
        }
    }
    template <class U>
    void dn6(U* x, const U* y) const {
        for (int q = 0; q < 6; ++q) {
            const U r = from(y[q], t < 63 ? t + 1 : t);
            if (t < 63) x[q] = r;
        }
    }
    template <class U>
    U lo_half(U v) const { return from(v, t & 31); }
    // device: v_permlane32_swap gives the lower half (own, partner), the upper (partner, own)
    template <class U>
    void xor32_pair(U v, U& a, U& b) const {
        const U o = from(v, t ^ 32);
        a = t < 32 ? v : o;
        b = t < 32 ? o : v;
    }
    template <class U>
    U uni_d(U v) const { return from(v, 0); }
    template <class U>
    U lane63(U v) const { return from(v, 63); }
    template <class U>
    U lane0(U v) const { return from(v, 0); }
    template <class U>
    U lanev(U v, int l) const { return from(v, l); }
    // reduction partners of the device (wave_dev.h): xor 1, xor 2, mirror 8, mirror 16, xor 16, xor 32
    template <int s, class U>
    U rpart(U v) const {
        const int p = s == 0 ? t ^ 1 : s == 1 ? t ^ 2 : s == 2 ? (t & ~7) | (7 - (t & 7))
                    : s == 3 ? (t & ~15) | (15 - (t & 15)) : s == 4 ? t ^ 16 : t ^ 32;
        return from(v, p);
    }
};

// ---------------------------------------------------------------- stdin
// The two parameter lines and the option lines up to "end" into P (Ipopt's defaults, no iteration
// budget, where a line is left out).  Returns the program's exit status: 0 to go on, 1 malformed
// input, 2 an unknown option name.
inline int read_params(mpcg::IpmParams& P) {
    P = mpcg::IpmParams{};
    mpcg::ipopt_default_options(P);
    P.cpu_iter_budget = -1;
    if (std::scanf("%d %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &P.N, &P.dt, &P.ref_cte,
                   &P.ref_eth, &P.ref_v, &P.w_cte, &P.w_eth, &P.w_v, &P.w_w, &P.w_a, &P.w_dw, &P.w_da, &P.max_w,
                   &P.max_a, &P.bound, &P.tol, &P.max_iter) != 17)
        return 1;
    if (std::scanf("%d %lf", &P.model, &P.lf) != 2) return 1;
    for (char key[64];;) {
        double v;
        if (std::scanf("%63s", key) != 1) return 1;
        if (!std::strcmp(key, "end")) return 0;
        if (std::scanf("%lf", &v) != 1) return 1;
        if (!std::strcmp(key, "cpu_iter_budget")) P.cpu_iter_budget = (int)v;
#define OPT_BY_NAME(type, field, name, dflt) else if (!std::strcmp(key, #name)) P.field = (type)v;
        MPCG_IPOPT_OPTIONS(OPT_BY_NAME)
#undef OPT_BY_NAME
        else {
            std::fprintf(stderr, "unknown option %s\n", key);
            return 2;
        }
    }
}

// n values of stdin as doubles ("nan" and "inf" included) into dst
template <class T>
bool read_values(T* dst, long n) {
    for (long i = 0; i < n; ++i) {
        double d;
        if (std::scanf("%lf", &d) != 1) return false;
        dst[i] = (T)d;
    }
    return true;
}

// B, then B x (state[6], coeffs[4]).  Returns 0, or 1 for malformed input.
inline int read_problems(std::vector<mpcg::IpmProblem<HT>>& probs) {
    long B;
    if (std::scanf("%ld", &B) != 1 || B < 0) return 1;
    probs.resize(B);
    for (auto& pr : probs)
        if (!read_values(pr.init, 6) || !read_values(pr.c, 4)) return 1;
    return 0;
}

// ---------------------------------------------------------------- a problem's memory
// What one wavefront of the device owns: the LDS image, its workspace slot (the spill argument of
// the first solver) and its park entry -- scalars, LDS image, then the workspace of the solver that
// continues it -- all NaN-filled: a value read before it is written shows.
struct Scratch {
    const mpcg::WideLayout L;
    HostShared sh;
    std::vector<HT> spill, park;
    Scratch(const mpcg::IpmParams& P, Fibers* fibers)
        : L(P.N, P.filter_cap, P.model), spill(L.slot(), (HT)std::nan("")), park(L.park(), (HT)std::nan("")) {
        sh.fib = fibers;
        sh.lds.assign(L.total(), std::nan(""));
    }
    HostWave wave(int t) { return HostWave{&sh, t, sh.lds.data()}; }
    const HT* image() const { return reinterpret_cast<const HT*>(sh.lds.data()); }
    // the 64 lanes of the problem: body(lane) on every fiber
    template <class F>
    void run(F& body) { sh.fib->run(body); }
};

// ---------------------------------------------------------------- the solver instance
// The WideSolver instance the device runs for (P.model, P.N) -- two stage blocks beyond N = 64, the
// split solver up to N = 32 -- constructed on the wave context wv and handed to f.  SPLIT_ONLY:
// the caller has refused N > 32, and only the two split instances are compiled.
template <bool SPLIT_ONLY = false, class WV, class F>
void with_solver(const mpcg::IpmParams& P, const mpcg::IpmProblem<HT>& pr, const WV& wv, Scratch& sc, F&& f) {
    auto go = [&]<int MODEL, bool SPLIT, int NB>() {
        mpcg::WideSolver<WV, MODEL, SPLIT, HT, NB> S(P, pr, wv, sc.spill.data());
        f(S);
    };
    if constexpr (SPLIT_ONLY) {
        if (P.model == 1)
            go.template operator()<1, true, 1>();
        else
            go.template operator()<0, true, 1>();
    } else {
        if (P.model == 1 && P.N > 64)
            go.template operator()<1, false, 2>();
        else if (P.model == 0 && P.N > 64)
            go.template operator()<0, false, 2>();
        else if (P.model == 1 && P.N <= 32)
            go.template operator()<1, true, 1>();
        else if (P.model == 1)
            go.template operator()<1, false, 1>();
        else if (P.N <= 32)
            go.template operator()<0, true, 1>();
        else
            go.template operator()<0, false, 1>();
    }
}

// A solve that ended with NEED_RESTO is parked and continued as the device's resume kernel does:
// a second solver of the same instance, its workspace inside the park entry, checks the entry,
// unparks it and finishes the restoration phase.  Called by all lanes after S0 ended; S2 is the
// caller's room for the second solver.  Returns the solver that holds the result.
template <class Solver>
Solver& continue_parked(Solver& S0, std::optional<Solver>& S2, Scratch& sc, long b) {
    if (S0.status != Solver::NEED_RESTO) return S0;
    HT* entry = sc.park.data();
    S2.emplace(S0.P, S0.pr, S0.wv, entry + Solver::PARK_SCALARS + sc.L.total());
    S0.park(entry, b);
    S0.wv.sync();
    if (!S2->park_entry_ok(entry, b)) {
        std::fprintf(stderr, "park entry check failed (problem %ld): tag %g nf %g iter %g n_resto %g\n", b,
                     (double)entry[Solver::PARK_TAG], (double)entry[11], (double)entry[10], (double)entry[25]);
        std::abort();
    }
    S2->unpark(entry);
    S2->finish_resto();
    return *S2;
}

// ---------------------------------------------------------------- the worker pool
// line(b, fibers) -> the output of problem b, on MPCG_HOST_THREADS workers (default the machine's
// CPUs, at least 1, at most B) that each own one Fibers and take the next problem; the outputs go
// to stdout in problem order.
template <class F>
void run_problems(long B, F&& line) {
    std::vector<std::string> out(B);
    const char* env = std::getenv("MPCG_HOST_THREADS");
    int nth = env ? std::atoi(env) : (int)std::thread::hardware_concurrency();
    nth = nth < 1 ? 1 : nth;
    if (nth > B) nth = (int)(B > 0 ? B : 1);
    std::atomic<long> next{0};
    auto worker = [&]() {
        auto fib = std::make_unique<Fibers>();
        for (long b; (b = next.fetch_add(1)) < B;) out[b] = line(b, fib.get());
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nth; ++i) pool.emplace_back(worker);
    worker();
    for (auto& x : pool) x.join();
    for (long b = 0; b < B; ++b) std::fputs(out[b].c_str(), stdout);
}

// ---------------------------------------------------------------- output lines
__attribute__((format(printf, 2, 3))) inline void append(std::string& line, const char* fmt, ...) {
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    line += buf;
}

// " %.17g" of every value (which round-trips: equal text, equal bits)
inline void append_values(std::string& line, const std::vector<double>& vals) {
    for (double v : vals) append(line, " %.17g", v);
}

// the final iterate: the LDS image [W(0), YP(0)) -- the records (w, z_L, z_U, dw) and y -- as hex
// words at the width of HT
inline void append_image(std::string& line, const Scratch& sc) {
    const HT* img = sc.image();
    for (int i = 0, n = sc.L.YP(0); i < n; ++i) {
        if constexpr (sizeof(HT) == 8) {
            uint64_t u;
            std::memcpy(&u, &img[i], 8);
            append(line, " %" PRIx64, u);
        } else {
            uint32_t u;
            std::memcpy(&u, &img[i], 4);
            append(line, " %" PRIx32, u);
        }
    }
}
