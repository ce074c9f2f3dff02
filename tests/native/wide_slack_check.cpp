// tests/native/wide_slack_check.cpp -- TEST HARNESS ONLY.
//
// The split solver's kept reciprocal slacks (mpc_ros_amd/csrc/wide_core.h, MPCG_FUSE bits 2
// and 3: the split accept pass and the statistics sweep keep rcp(w - lo), rcp(hi - w) of their
// lane's four variables, and the statistics, the step statistics and the next accept pass at
// the same iterate take them instead of forming them again) against the build without them:
// this file is compiled as it stands and with -DMPCG_FUSE=3, and
// tests/test_slack_cache_host.py demands that the two programs print the same bytes for the
// same input: statuses, iteration counts and the final iterate (w, z_L, z_U, the step, y) bit
// for bit.
//
// The 64 lanes are the fibers of wide_host_check.cpp (its source is included, its main
// renamed); the wavefront context here counts the consumer sweeps: at forward()'s mark the
// step-statistics sweeps that took the kept reciprocals (mark 18) and those that formed them
// (mark 19), at stats_split()'s mark the statistics sweeps that took the pair of the split
// accept pass before them (mark 21) and those that formed their own (mark 16).
//
// stdin: as wide_host_check.cpp.  -DHOST_T=float: the fp32 split solver (keeps none).
// stdout: per problem "status iters retries" (retries: Newton solves repeated by the inertia
//         correction) and the LDS image [W(0), YP(0)) as hex words; then one line
//         "sweeps <all> cached <n>".
#define main wide_host_check_main
#include "wide_host_check.cpp"
#undef main

#include <cinttypes>

struct CountWave : HostWave {
    // [4]: consumer sweeps that took the kept reciprocal slacks, sweeps that formed them
    // (the original problem's: the split solver marks them), solves that ended (k_newton), line
    // searches begun (ls_begin)
    long* cnt;
    void mark(int id) const {
        if (t != 0) return;
        if (id == 18 || id == 19) ++cnt[id - 18];
        if (id == 21 || id == 16) ++cnt[id == 21 ? 0 : 1];  // (the statistics sweep as a consumer: after the split accept pass / forming its own)
        if (id == 11 || id == 12) ++cnt[id - 9];
    }
};

int main() {
    mpcg::IpmParams P{};
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
        if (!std::strcmp(key, "end")) break;
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
    if (P.N > 32) {
        std::fprintf(stderr, "the split solver takes N <= 32\n");
        return 2;
    }
    long B;
    if (std::scanf("%ld", &B) != 1) return 1;
    const mpcg::WideLayout L(P.N, P.filter_cap, P.model);
    std::vector<mpcg::IpmProblem<HT>> probs(B);
    for (long b = 0; b < B; ++b) {
        for (HT& v : probs[b].init) { double d; if (std::scanf("%lf", &d) != 1) return 1; v = (HT)d; }
        for (HT& v : probs[b].c) { double d; if (std::scanf("%lf", &d) != 1) return 1; v = (HT)d; }
    }
    std::vector<std::string> out(B);
    std::vector<long> counts(4 * B, 0);
    const int nimg = L.YP(0);  // the records (w, z_L, z_U, dw) and y
    auto solve_one = [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        HostShared sh;
        sh.lds.assign(L.total(), std::nan(""));
        std::vector<HT> spill(L.slot(), (HT)std::nan(""));
        std::vector<HT> park(32 + L.total() + L.slot(), (HT)std::nan(""));
        int status = 0, iters = 0;
        auto lane = [&](int t) {
            CountWave wv{{&sh, t, sh.lds.data()}, &counts[4 * b]};
            auto run = [&](auto& S0) {
                typedef std::decay_t<decltype(S0)> Solver;
                S0.solve();
                // a restoration phase: parked and continued as the device's second kernel does
                Solver S2(P, pr, wv, park.data() + Solver::PARK_SCALARS + L.total());
                const bool parked = S0.status == Solver::NEED_RESTO;
                if (parked) {
                    S0.park(park.data(), b);
                    wv.sync();
                    if (!S2.park_entry_ok(park.data(), b)) std::abort();
                    S2.unpark(park.data());
                    S2.finish_resto();
                }
                Solver& S = parked ? S2 : S0;
                wv.sync();
                if (t == 0) {
                    status = S.status;
                    iters = S.iter;
                }
            };
            if (P.model == 1) {
                mpcg::WideSolver<CountWave, 1, true, HT> S(P, pr, wv, spill.data());
                run(S);
            } else {
                mpcg::WideSolver<CountWave, 0, true, HT> S(P, pr, wv, spill.data());
                run(S);
            }
        };
        sh.fib = fibers;
        sh.fib->run(lane);
        std::string line;
        char buf[64];
        // (a solve that does not reach the line search: an inertia-correction retry, or -- once per
        // restoration phase at most -- the perturbation's limit)
        std::snprintf(buf, sizeof buf, "%d %d %ld", status, iters, counts[4 * b + 2] - counts[4 * b + 3]);
        line += buf;
        const HT* img = reinterpret_cast<const HT*>(sh.lds.data());
        for (int i = 0; i < nimg; ++i) {
            if (sizeof(HT) == 8) {
                uint64_t u;
                std::memcpy(&u, &img[i], 8);
                std::snprintf(buf, sizeof buf, " %" PRIx64, u);
            } else {
                uint32_t u;
                std::memcpy(&u, &img[i], 4);
                std::snprintf(buf, sizeof buf, " %" PRIx32, u);
            }
            line += buf;
        }
        line += "\n";
        out[b] = line;
    };
    const char* env = std::getenv("MPCG_HOST_THREADS");
    int nth = env ? std::atoi(env) : (int)std::thread::hardware_concurrency();
    nth = nth < 1 ? 1 : nth;
    if (nth > B) nth = (int)(B > 0 ? B : 1);
    std::atomic<long> next{0};
    auto worker = [&]() {
        auto fib = std::make_unique<Fibers>();
        for (long b; (b = next.fetch_add(1)) < B;) solve_one(b, fib.get());
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nth; ++i) pool.emplace_back(worker);
    worker();
    for (auto& x : pool) x.join();
    long cached = 0, formed = 0;
    for (long b = 0; b < B; ++b) {
        std::fputs(out[b].c_str(), stdout);
        cached += counts[4 * b];
        formed += counts[4 * b + 1];
    }
    std::printf("sweeps %ld cached %ld\n", cached + formed, cached);
    return 0;
}
