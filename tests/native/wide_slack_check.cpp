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
// The 64 lanes are the fibers of host_wave.h; the wavefront context here counts the consumer
// sweeps: at forward()'s mark the step-statistics sweeps that took the kept reciprocals (mark
// 18) and those that formed them (mark 19), at stats_split()'s mark the statistics sweeps that
// took the pair of the split accept pass before them (mark 21) and those that formed their own
// (mark 16).
//
// stdin: as host_wave.h; N > 32 is refused (exit status 2).  -DHOST_T=float: the fp32 split
//        solver (keeps none).
// stdout: per problem "status iters retries" (retries: Newton solves repeated by the inertia
//         correction) and the LDS image [W(0), YP(0)) as hex words; then one line
//         "sweeps <all> cached <n>".
#include "host_wave.h"

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
    mpcg::IpmParams P;
    std::vector<mpcg::IpmProblem<HT>> probs;
    if (int rc = read_params(P)) return rc;
    if (P.N > 32) {
        std::fprintf(stderr, "the split solver takes N <= 32\n");
        return 2;
    }
    if (int rc = read_problems(probs)) return rc;
    const long B = (long)probs.size();
    std::vector<long> counts(4 * B, 0);
    run_problems(B, [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        Scratch sc(P, fibers);
        int status = 0, iters = 0;
        auto lane = [&](int t) {
            CountWave wv{sc.wave(t), &counts[4 * b]};
            with_solver<true>(P, pr, wv, sc, [&](auto& S0) {
                S0.solve();
                std::optional<std::decay_t<decltype(S0)>> S2;
                auto& S = continue_parked(S0, S2, sc, b);
                wv.sync();
                if (t == 0) {
                    status = S.status;
                    iters = S.iter;
                }
            });
        };
        sc.run(lane);
        std::string line;
        // (a solve that does not reach the line search: an inertia-correction retry, or -- once per
        // restoration phase at most -- the perturbation's limit)
        append(line, "%d %d %ld", status, iters, counts[4 * b + 2] - counts[4 * b + 3]);
        append_image(line, sc);
        return line + "\n";
    });
    long cached = 0, formed = 0;
    for (long b = 0; b < B; ++b) {
        cached += counts[4 * b];
        formed += counts[4 * b + 1];
    }
    std::printf("sweeps %ld cached %ld\n", cached + formed, cached);
    return 0;
}
