// tests/native/wide_start_check.cpp -- TEST HARNESS ONLY.
//
// A solve started from a solution record (mpc_ros_amd/csrc/wide_core.h WideSolver::init_start)
// on the host: the one-problem-per-wavefront solver on the 64 fibers of wide_host_check.cpp (its
// source is included, its main renamed), started by init_start in the mode of each problem, every
// ending followed by the epilogue the device's write_out runs.  A problem that needs the
// restoration phase is parked and continued as the device's resume kernel does.
// tests/test_start_host.py compares the outputs with the cold solve and the oracle.
//
// stdin: as wide_sol_check.cpp up to the problems, then one integer (1: the negative control --
//        after init_start the scaling is replaced by the cold setup()'s), then per problem
//        "mode mu0" and the start record, 3 (8N - 2) + 6N doubles.
// stdout: per problem one line "status iters used n_resto n_fover nf_peak sf obj u0[2] traj[3N]
//         sol[3 (8N - 2) + 6N]", every double as %.17g (equal text, equal bits).
#define main wide_host_check_main
#include "wide_host_check.cpp"
#undef main

int main() {
    static_assert(std::is_same_v<HT, double>, "the record is the fp64 solver's");
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
    long B;
    if (std::scanf("%ld", &B) != 1) return 1;
    const mpcg::WideLayout L(P.N, P.filter_cap, P.model);
    std::vector<mpcg::IpmProblem<HT>> probs(B);
    for (long b = 0; b < B; ++b) {
        for (HT& v : probs[b].init) { double d; if (std::scanf("%lf", &d) != 1) return 1; v = (HT)d; }
        for (HT& v : probs[b].c) { double d; if (std::scanf("%lf", &d) != 1) return 1; v = (HT)d; }
    }
    int cold_scaling = 0;
    if (std::scanf("%d", &cold_scaling) != 1) return 1;
    const long ne = (long)mpcg::solution_elems(P.N);
    std::vector<int> modes(B);
    std::vector<double> mu0s(B), starts((size_t)B * ne);
    for (long b = 0; b < B; ++b) {
        if (std::scanf("%d %lf", &modes[b], &mu0s[b]) != 2) return 1;
        // (%lf reads "nan" and "inf": a caller's bad start)
        for (long e = 0; e < ne; ++e)
            if (std::scanf("%lf", &starts[(size_t)b * ne + e]) != 1) return 1;
    }
    std::vector<std::string> out(B);
    auto solve_one = [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        HostShared sh;
        sh.lds.assign(L.total(), std::nan(""));
        std::vector<HT> spill(L.slot(), (HT)std::nan(""));
        std::vector<HT> park(32 + L.total() + L.slot(), (HT)std::nan(""));
        std::vector<double> rec(3 + 3 * P.N, 0.0), sol(ne, std::nan(""));
        int status = 0, iters = 0, used = 0, dg[3] = {0, 0, 0};
        double sf = 0;
        auto lane = [&](int t) {
            HostWave wv{&sh, t, sh.lds.data()};
            auto run = [&](auto& S0) {
                typedef std::decay_t<decltype(S0)> Solver;
                const int u = S0.init_start(starts.data() + (size_t)b * ne, modes[b], (HT)mu0s[b]);
                if (cold_scaling) {
                    wv.sync();
                    S0.setup();
                    wv.sync();
                }
                S0.run();
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
                const double o = S.objective_out();
                if (t == 0) {
                    status = S.status;
                    iters = S.iter;
                    used = u;
                    dg[0] = S.n_resto;
                    dg[1] = S.n_fover;
                    dg[2] = S.nf_peak;
                    sf = (double)S.sf;
                    rec[0] = o;
                    rec[1] = S.x_ctrl(0, 0);
                    rec[2] = S.x_ctrl(1, 0);
                    for (int s = 0; s < 3; ++s)
                        for (int k = 0; k < P.N; ++k) rec[3 + s * P.N + k] = S.x_state(s, k);
                }
                S.solution_out(sol.data());
                wv.sync();
            };
            if (P.model == 1 && P.N > 64) {
                mpcg::WideSolver<HostWave, 1, false, HT, 2> S(P, pr, wv, spill.data());
                run(S);
            } else if (P.model == 0 && P.N > 64) {
                mpcg::WideSolver<HostWave, 0, false, HT, 2> S(P, pr, wv, spill.data());
                run(S);
            } else if (P.model == 1 && P.N <= 32) {
                mpcg::WideSolver<HostWave, 1, true, HT> S(P, pr, wv, spill.data());
                run(S);
            } else if (P.model == 1) {
                mpcg::WideSolver<HostWave, 1, false, HT> S(P, pr, wv, spill.data());
                run(S);
            } else if (P.N <= 32) {
                mpcg::WideSolver<HostWave, 0, true, HT> S(P, pr, wv, spill.data());
                run(S);
            } else {
                mpcg::WideSolver<HostWave, 0, false, HT> S(P, pr, wv, spill.data());
                run(S);
            }
        };
        sh.fib = fibers;
        sh.fib->run(lane);
        std::string line;
        char buf[96];
        std::snprintf(buf, sizeof buf, "%d %d %d %d %d %d %.17g", status, iters, used, dg[0], dg[1], dg[2], sf);
        line += buf;
        for (double v : rec) {
            std::snprintf(buf, sizeof buf, " %.17g", v);
            line += buf;
        }
        for (double v : sol) {
            std::snprintf(buf, sizeof buf, " %.17g", v);
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
    for (long b = 0; b < B; ++b) std::fputs(out[b].c_str(), stdout);
    return 0;
}
