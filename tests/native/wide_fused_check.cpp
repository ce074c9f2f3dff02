// tests/native/wide_fused_check.cpp -- TEST HARNESS ONLY.
//
// The split solver's fused sweeps (mpc_ros_amd/csrc/wide_core.h, MPCG_FUSE) against its
// separate passes: this file is compiled twice, once as it stands (the fused sweeps: the
// statistics sweep writes the Newton system's stage data and reuses an accepted trial
// point's sums) and once with -DMPCG_FUSE=0 (precompute_split on every solve, every sum
// evaluated again), and tests/test_fused_sweeps_host.py demands that the two programs
// print the same bytes for the same input: statuses, iteration counts and the final
// iterate (w, z_L, z_U, the step, y) bit for bit.
//
// The 64 lanes are the fibers of host_wave.h; the wavefront context here counts, at
// riccati()'s mark, the Newton solves that skipped the stage-data pass (mark 14) and those
// that ran it (mark 15).
//
// stdin: as host_wave.h; N > 32 is refused (exit status 2).  -DHOST_T=float: the fp32 split solver.
// stdout: per problem "status iters retries" (retries: Newton solves repeated by the inertia
//         correction) and the LDS image [W(0), YP(0)) as hex words; then one line
//         "solves <all> skipped <n>".
#include "host_wave.h"

struct CountWave : HostWave {
    // [4]: solves that skipped the stage-data pass, solves that ran it (the original problem's:
    // the split solver marks them), solves that ended (k_newton), line searches begun (ls_begin)
    long* cnt;
    void mark(int id) const {
        if (t != 0) return;
        if (id == 14 || id == 15) ++cnt[id - 14];
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
    long skipped = 0, ran = 0;
    for (long b = 0; b < B; ++b) {
        skipped += counts[4 * b];
        ran += counts[4 * b + 1];
    }
    std::printf("solves %ld skipped %ld\n", skipped + ran, skipped);
    return 0;
}
