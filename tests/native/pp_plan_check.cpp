// tests/native/pp_plan_check.cpp -- the per-problem instances of the launch plan
// (mpc_ros_amd/csrc/wide_plan.h pp_solve_key / pp_resume_key, MPCG_WIDE_PP_*_INSTANCES) on the
// host; no GPU runtime.  Exit status 1 and a message at the first property that fails; prints
// the per-problem solve instance chosen under a non-default option per (model, horizon range).
//
//   g++ -std=c++20 -o pp_plan_check tests/native/pp_plan_check.cpp && ./pp_plan_check
#include <cstdio>
#include <cstdlib>
#include <string>

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

#define NAME7(g, M, S, T, NB, D, W) MPCG_PP_SOLVE_NAME(M, S, T, NB, D, W),
static const char* const kNames[] = {MPCG_WIDE_PP_SOLVE_INSTANCES(NAME7)};

template <size_t n>
static int index_of(const WideKey (&keys)[n], const WideKey& k) {
    for (size_t i = 0; i < n; ++i)
        if (keys[i] == k) return (int)i;
    return -1;
}

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

int main() {
    constexpr size_t ns = sizeof(kPPSolveKeys) / sizeof(WideKey), nr = sizeof(kPPResumeKeys) / sizeof(WideKey);
    static_assert(sizeof(kNames) / sizeof(kNames[0]) == ns);
    bool used_s[ns] = {}, used_r[nr] = {};
    for (int model = 0; model < 2; ++model) {
        std::string cur;
        int from = 1;
        for (int N = 1; N <= 129; ++N) {
            std::string name = "END";
            for (int opt = 0; opt < 2 && N <= 128; ++opt)
                for (long B : {1L, 4096L, 4097L}) {
                    const IpmParams P = params(N, model, 0, opt);
                    const WideKey k = pp_solve_key(P, B);
                    CHECK(k.ok(), "model %d N %d", model, N);
                    const int i = index_of(kPPSolveKeys, k);
                    CHECK(i >= 0, "per-problem solve key of model %d N %d option %d B %ld not in the list", model, N, opt, B);
                    used_s[i] = true;
                    // fp64, the class and register allocation of the plain general instance; the
                    // default-options instance only under default options
                    const WideKey plain = solve_key(params(N, model, 0, true), 4097);
                    CHECK(!k.f32 && k.model == plain.model && k.split == plain.split && k.nb == plain.nb &&
                              k.wpe == plain.wpe && (!k.defopt || !opt),
                          "model %d N %d: not the plain general instance's class", model, N);
                    const WideKey rk = pp_resume_key(P);
                    const int r = index_of(kPPResumeKeys, rk);
                    CHECK(r >= 0 && rk == resume_key(P), "per-problem resume key of model %d N %d", model, N);
                    used_r[r] = true;
                    if (opt) name = kNames[i];
                    // fp32 is refused
                    const IpmParams P32 = params(N, model, 1, opt);
                    CHECK(!pp_solve_key(P32, B).ok() && !pp_resume_key(P32).ok(), "fp32 model %d N %d", model, N);
                }
            if (N == 1) cur = name;
            if (name != cur) {
                std::printf("model %d N %d..%d %s\n", model, from, N - 1, cur.c_str());
                cur = name;
                from = N;
            }
        }
    }
    for (size_t i = 0; i < ns; ++i) CHECK(used_s[i], "per-problem solve instance %s is never chosen", kNames[i]);
    for (size_t i = 0; i < nr; ++i) CHECK(used_r[i], "per-problem resume instance %zu is never chosen", i);
    CHECK(!pp_solve_key(params(129, 0, 0, false), 1).ok() && !pp_resume_key(params(129, 0, 0, false)).ok(), "N = 129");
    return 0;
}
