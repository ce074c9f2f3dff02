// tests/native/wide_start_check.cpp -- TEST HARNESS ONLY.
//
// A solve started from a solution record (mpc_ros_amd/csrc/wide_core.h WideSolver::init_start)
// on the host: the one-problem-per-wavefront solver on the 64 fibers of host_wave.h, started by
// init_start in the mode of each problem, every ending followed by the epilogue the device's
// write_out runs.  A problem that needs the restoration phase is parked and continued as the
// device's resume kernel does.
// tests/test_start_host.py compares the outputs with the cold solve and the oracle.
//
// stdin: as host_wave.h (double only), then one integer (1: the negative control -- after
//        init_start the scaling is replaced by the cold setup()'s), then per problem "mode mu0"
//        and the start record, 3 (8N - 2) + 6N doubles.
// stdout: per problem one line "status iters used n_resto n_fover nf_peak sf obj u0[2] traj[3N]
//         sol[3 (8N - 2) + 6N]", every double as %.17g (equal text, equal bits).
#include "host_wave.h"

int main() {
    static_assert(std::is_same_v<HT, double>, "the record is the fp64 solver's");
    mpcg::IpmParams P;
    std::vector<mpcg::IpmProblem<HT>> probs;
    if (int rc = read_params(P)) return rc;
    if (int rc = read_problems(probs)) return rc;
    const long B = (long)probs.size();
    int cold_scaling = 0;
    if (std::scanf("%d", &cold_scaling) != 1) return 1;
    const long ne = (long)mpcg::solution_elems(P.N);
    std::vector<int> modes(B);
    std::vector<double> mu0s(B), starts((size_t)B * ne);
    for (long b = 0; b < B; ++b) {
        if (std::scanf("%d %lf", &modes[b], &mu0s[b]) != 2) return 1;
        // ("nan" and "inf" are read: a caller's bad start)
        if (!read_values(&starts[(size_t)b * ne], ne)) return 1;
    }
    run_problems(B, [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        Scratch sc(P, fibers);
        std::vector<double> rec(3 + 3 * P.N, 0.0), sol(ne, std::nan(""));
        int status = 0, iters = 0, used = 0, dg[3] = {0, 0, 0};
        double sf = 0;
        auto lane = [&](int t) {
            HostWave wv = sc.wave(t);
            with_solver(P, pr, wv, sc, [&](auto& S0) {
                const int u = S0.init_start(starts.data() + (size_t)b * ne, modes[b], (HT)mu0s[b]);
                if (cold_scaling) {
                    wv.sync();
                    S0.setup();
                    wv.sync();
                }
                S0.run();
                std::optional<std::decay_t<decltype(S0)>> S2;
                auto& S = continue_parked(S0, S2, sc, b);
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
            });
        };
        sc.run(lane);
        std::string line;
        append(line, "%d %d %d %d %d %d %.17g", status, iters, used, dg[0], dg[1], dg[2], sf);
        append_values(line, rec);
        append_values(line, sol);
        return line + "\n";
    });
    return 0;
}
