// tests/native/wide_ric_check.cpp -- TEST HARNESS ONLY.
//
// The Riccati sweep with the affine part p as a ninth column of its lane grid
// (mpc_ros_amd/csrc/wide_core.h, MPCG_RIC9: riccati9()) against the sweep in which every lane
// of a row forms p_i (riccati()'s own body): this file is compiled as it stands and with
// -DMPCG_RIC9=0, and tests/test_riccati_lanes_host.py demands that the two programs print the
// same bytes for the same input: statuses, iteration counts, the final iterate (w, z_L, z_U,
// the step, y) bit for bit, and a running hash of the gain records of every sweep -- an
// indexing slip shows there even where the solve converges anyway.
//
// The 64 lanes are the fibers of host_wave.h.  The wavefront context here hashes, at the mark
// that ends a sweep (mark 2), the 18 values per stage (K[0][0..7], K[1][0..7], kff[2]) of
// stages 0..N-2 where WideSolver::ld_gains reads them: the LDS records KR(k), or (KL = 0: the
// bicycle, N > 32) the workspace records SP_KRG of the problem's slot and of its park entry's
// (the solver that continues a parked problem writes there).  Lane 63 hashes: the fibers run in
// lane order, so every other lane's last stores of the sweep are done.  The restoration
// problem's sweeps reach the same mark; what the records hold then is hashed as well.
//
// stdin: as host_wave.h.  -DHOST_T=float: the fp32 solver (riccati()'s body under either setting).
// stdout: per problem "status iters retries hash" (retries: Newton solves repeated by the
//         inertia correction; hash: FNV-1a over the records' bytes, hex) and the LDS image
//         [W(0), YP(0)) as hex words; then one line "sweeps <n>".
#include "host_wave.h"

struct RicWave : HostWave {
    const Scratch* sc;
    uint64_t* hash;
    long* cnt;  // [3]: sweeps ended, solves that ended (k_newton), line searches begun (ls_begin)
    void bytes(const HT* p, int n) const {
        const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
        for (size_t q = 0; q < n * sizeof(HT); ++q) *hash = (*hash ^ b[q]) * 1099511628211ull;
    }
    void mark(int id) const {
        if (id == 2 && t == 63) {
            const mpcg::WideLayout& L = sc->L;
            for (int k = 0; k + 1 < L.N; ++k) {
                if (L.KL != 0) {
                    bytes(sc->image() + L.KR(k), mpcg::WideLayout::KS);
                } else {
                    bytes(sc->spill.data() + L.SP_KRG() + mpcg::WideLayout::KS * k, mpcg::WideLayout::KS);
                    bytes(sc->park.data() + mpcg::WideLayout::PARK_SCALARS + L.total() + L.SP_KRG() +
                              mpcg::WideLayout::KS * k,
                          mpcg::WideLayout::KS);
                }
            }
            ++cnt[0];
        }
        if (t != 0) return;
        if (id == 11 || id == 12) ++cnt[id - 10];
    }
};

int main() {
    mpcg::IpmParams P;
    std::vector<mpcg::IpmProblem<HT>> probs;
    if (int rc = read_params(P)) return rc;
    if (int rc = read_problems(probs)) return rc;
    const long B = (long)probs.size();
    std::vector<long> counts(3 * B, 0);
    run_problems(B, [&](long b, Fibers* fibers) {
        const mpcg::IpmProblem<HT> pr = probs[b];
        Scratch sc(P, fibers);
        int status = 0, iters = 0;
        uint64_t hash = 14695981039346656037ull;
        auto lane = [&](int t) {
            RicWave wv{sc.wave(t), &sc, &hash, &counts[3 * b]};
            with_solver(P, pr, wv, sc, [&](auto& S0) {
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
        append(line, "%d %d %ld %" PRIx64, status, iters, counts[3 * b + 1] - counts[3 * b + 2], hash);
        append_image(line, sc);
        return line + "\n";
    });
    long sweeps = 0;
    for (long b = 0; b < B; ++b) sweeps += counts[3 * b];
    std::printf("sweeps %ld\n", sweeps);
    return 0;
}
