// tests/native/wide_sol_check.cpp -- TEST HARNESS ONLY.
//
// The solver's solution record (mpc_ros_amd/csrc/wide_core.h WideSolver::solution_out) on the
// host: the one-problem-per-wavefront solver on the 64 fibers of host_wave.h, every ending
// followed by the epilogue the device's write_out runs -- the outputs through x_ctrl / x_state /
// objective_out, then solution_out by all lanes.
// tests/test_solution_host.py compares the records with the oracle.
//
// stdin: as host_wave.h (double only).
// stdout: per problem one line "status iters obj u0[2] traj[3N] sol[3 (8N - 2) + 6N]", every
//         double as %.17g (which round-trips: equal text, equal bits).
#include "host_wave.h"

int main() {
    static_assert(std::is_same_v<HT, double>, "the record is the fp64 solver's");
    mpcg::IpmParams P;
    std::vector<mpcg::IpmProblem<HT>> probs;
    if (int rc = read_params(P)) return rc;
    if (int rc = read_problems(probs)) return rc;
    const long ne = (long)mpcg::solution_elems(P.N);
    run_problems((long)probs.size(), [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        Scratch sc(P, fibers);
        std::vector<double> rec(3 + 3 * P.N, 0.0), sol(ne, std::nan(""));
        int status = 0, iters = 0;
        auto lane = [&](int t) {
            HostWave wv = sc.wave(t);
            with_solver(P, pr, wv, sc, [&](auto& S0) {
                S0.solve();
                std::optional<std::decay_t<decltype(S0)>> S2;
                auto& S = continue_parked(S0, S2, sc, b);
                const double o = S.objective_out();
                if (t == 0) {
                    status = S.status;
                    iters = S.iter;
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
        append(line, "%d %d", status, iters);
        append_values(line, rec);
        append_values(line, sol);
        return line + "\n";
    });
    return 0;
}
