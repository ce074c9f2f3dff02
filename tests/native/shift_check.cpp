// tests/native/shift_check.cpp -- TEST HARNESS ONLY.
//
// A stand-alone program over mpc_ros_amd/csrc/mpcg_shift.h (the shift rule and its host loop),
// built with -fsanitize=address,undefined and run directly by tests/test_shift_host.py: every index
// the rule forms (the record's four parts, the two control blocks, the held last entries, the
// terminal step's operands) is exercised at the horizons where the cases differ -- N = 2 (one
// control, held), 3, 64, 65 and 128 -- on exactly sized heap arrays, for both models, out of place
// and in place.
//
// Checked here without a second statement of the rule's arithmetic: stage 0 is the new state; the
// moved entries are the source's, bit for bit; under zero motion the mapped entries are moved ones
// too; the terminal stage has zero defect as kkt_stage evaluates it (the primal column of the
// certificate of the shifted record's last two stages); in place equals out of place bit for bit.
// The numbers against an independent restatement: tests/test_shift_host.py.  Prints "ok" and exits
// 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpcg_shift.h"

static int fails = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "line %d (N %d model %d): %s\n", __LINE__, N, model, #c); \
            ++fails;                                                               \
        }                                                                          \
    } while (0)

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void one(int N, int model, bool zero_motion) {
    double r[MPCG_PP_FIELDS] = {};
    r[MPCG_PP_DT] = 0.1;
    r[MPCG_PP_REF_V] = 0.5;
    r[MPCG_PP_ANGVEL] = 3;
    r[MPCG_PP_MAXTHR] = 1;
    r[MPCG_PP_BOUND] = 1000;
    r[MPCG_PP_LF] = 0.5;
    const double state[6] = {0.01, -0.02, 0.05, 0.4, 0.3, -0.1}, c[4] = {0.2, 0.1, -0.05, 0.01};
    const double motion[3] = {zero_motion ? 0.0 : 0.04, zero_motion ? 0.0 : -0.003, zero_motion ? 0.0 : 3.1};
    const int nx = 8 * N - 2, ne = mpcg::shift_record_elems(N);
    std::vector<double> src((size_t)ne), out((size_t)ne), work((size_t)ne);  // (exactly the record)
    for (int e = 0; e < ne; ++e) src[e] = std::sin(0.37 * e + N) + 1e-3 * e;
    mpcg::shift_problem(r, model, N, state, c, motion, src.data(), out.data(), work.data());
    const double *x = src.data(), *o = out.data();
    for (int s = 0; s < 6; ++s) {
        CHECK(same(o[s * N], state[s]));
        for (int k = 1; k <= N - 2; ++k)
            if (s >= 3 || zero_motion) CHECK(same(o[s * N + k], x[s * N + k + 1]));
    }
    for (int part = 0; part < 3; ++part) {
        const double *xs = x + part * nx, *os = o + part * nx;
        for (int j = 0; j < 2; ++j) {
            const int base = 6 * N + j * (N - 1);
            for (int k = 0; k <= N - 3; ++k) CHECK(same(os[base + k], xs[base + k + 1]));
            CHECK(same(os[base + N - 2], xs[base + N - 2]));
        }
        if (part == 0) continue;
        for (int s = 0; s < 6; ++s) {
            for (int k = 0; k <= N - 2; ++k) CHECK(same(os[s * N + k], xs[s * N + k + 1]));
            CHECK(same(os[s * N + N - 1], xs[s * N + N - 1]));
        }
    }
    const double *lam = x + 3 * nx, *ol = o + 3 * nx;
    for (int s = 0; s < 6; ++s)
        for (int k = 0; k < N; ++k)
            if (s >= 2 || zero_motion) CHECK(same(ol[s * N + k], lam[s * N + (k + 1 < N ? k + 1 : N - 1)]));
    // the last dynamics step of the shifted record: zero defect as kkt_stage evaluates it
    {
        double s[6], sp[6], up[2], z[8] = {}, l[6] = {}, u[2] = {}, ln[6] = {}, un[2] = {};
        for (int j = 0; j < 6; ++j) {
            s[j] = o[j * N + N - 1];
            sp[j] = o[j * N + N - 2];
        }
        up[0] = o[6 * N + N - 2];
        up[1] = o[7 * N - 1 + N - 2];
        const mpcg::KktCert cert = mpcg::kkt_stage(r, model, N, N - 1, c, state, s, u, z, z, l, sp, up, ln, un);
        CHECK(cert.prim == 0.0);
    }
    // in place
    std::vector<double> ip(src);
    mpcg::shift_problem(r, model, N, state, c, motion, ip.data(), ip.data(), work.data());
    CHECK(std::memcmp(ip.data(), out.data(), sizeof(double) * (size_t)ne) == 0);
}

int main() {
    for (int model = 0; model < 2; ++model)
        for (int N : {2, 3, 64, 65, 128})
            for (int z = 0; z < 2; ++z) one(N, model, z != 0);
    if (fails) return 1;
    std::puts("ok");
    return 0;
}
