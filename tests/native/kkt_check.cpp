// tests/native/kkt_check.cpp -- TEST HARNESS ONLY.
//
// A stand-alone program over mpc_ros_amd/csrc/mpcg_kkt.h (the KKT certificate's stage body and its
// host loop), built with -fsanitize=address,undefined and run directly by tests/test_kkt_host.py:
// every index the host loop forms (the record's four parts, the neighbouring stages, the two
// control blocks) is exercised at the horizons where the cases differ -- N = 2 (no rate term, one
// control), 3 (one rate term), 20, 64, 65 and 128 -- on exactly sized heap arrays, for both models.
//
// The records are built here, not solved: a rollout of the dynamics from the initial state under
// given controls is feasible, so column 1 must be rounding; with lambda = z = 0 column 0 is the
// largest |grad f| and column 2 is 0; column 3 is the cost summed here directly.  An invalid
// parameter row gives NaN in all four columns.  Prints "ok" and exits 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mpcg_kkt.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static void one(int N, int model) {
    double r[MPCG_PP_FIELDS] = {};
    r[MPCG_PP_DT] = 0.1;
    r[MPCG_PP_REF_V] = 0.5;
    r[MPCG_PP_W_CTE] = 100;
    r[MPCG_PP_W_EPSI] = 100;
    r[MPCG_PP_W_V] = 1;
    r[MPCG_PP_W_ANGVEL] = 10;
    r[MPCG_PP_W_A] = 5;
    r[MPCG_PP_W_DANGVEL] = 3;
    r[MPCG_PP_W_DA] = 2;
    r[MPCG_PP_ANGVEL] = 3;
    r[MPCG_PP_MAXTHR] = 1;
    r[MPCG_PP_BOUND] = 1000;
    r[MPCG_PP_LF] = 0.5;
    const double init[6] = {0.1, -0.2, 0.05, 0.4, 0.3, -0.1}, c[4] = {0.2, 0.1, -0.05, 0.01};
    const int nx = 8 * N - 2;
    std::vector<double> sol(3 * nx + 6 * N, 0.0);  // (exactly the record: an index past it is an ASan report)
    double* x = sol.data();
    for (int j = 0; j < 6; ++j) x[j * N] = init[j];
    double f = 0, gmax = 0;
    for (int k = 0; k < N; ++k) {
        double s[6];
        for (int j = 0; j < 6; ++j) s[j] = x[j * N + k];
        f += r[MPCG_PP_W_CTE] * s[4] * s[4] + r[MPCG_PP_W_EPSI] * s[5] * s[5] +
             r[MPCG_PP_W_V] * (s[3] - 0.5) * (s[3] - 0.5);
        gmax = std::fmax(gmax, std::fmax(std::fabs(2 * r[MPCG_PP_W_CTE] * s[4]),
                                         std::fmax(std::fabs(2 * r[MPCG_PP_W_EPSI] * s[5]),
                                                   std::fabs(2 * r[MPCG_PP_W_V] * (s[3] - 0.5)))));
        if (k == N - 1) break;
        const double w = 0.3 * std::sin(0.7 * k), a = 0.2 * std::cos(0.3 * k);
        x[6 * N + k] = w;
        x[7 * N - 1 + k] = a;
        const double turn = model == 1 ? s[3] * w / r[MPCG_PP_LF] * 0.1 : w * 0.1;
        const double fx = c[0] + c[1] * s[0] + c[2] * s[0] * s[0] + c[3] * s[0] * s[0] * s[0];
        x[0 * N + k + 1] = s[0] + s[3] * std::cos(s[2]) * 0.1;
        x[1 * N + k + 1] = s[1] + s[3] * std::sin(s[2]) * 0.1;
        x[2 * N + k + 1] = s[2] + turn;
        x[3 * N + k + 1] = s[3] + a * 0.1;
        x[4 * N + k + 1] = (fx - s[1]) + s[3] * std::sin(s[5]) * 0.1;
        x[5 * N + k + 1] = s[5] + turn;
    }
    for (int k = 0; k < N - 1; ++k) {
        const double w = x[6 * N + k], a = x[7 * N - 1 + k];
        f += r[MPCG_PP_W_ANGVEL] * w * w + r[MPCG_PP_W_A] * a * a;
        if (k < N - 2) {
            const double dw = x[6 * N + k + 1] - w, da = x[7 * N - 1 + k + 1] - a;
            f += r[MPCG_PP_W_DANGVEL] * dw * dw + r[MPCG_PP_W_DA] * da * da;
        }
    }
    mpcg::KktCert o = mpcg::kkt_problem(r, model, N, init, c, sol.data());
    CHECK(o.prim <= 1e-13);
    CHECK(o.comp == 0.0);
    CHECK(o.stat >= gmax);  // (lambda = z = 0: the gradient itself, the controls' included)
    CHECK(std::fabs(o.f - f) <= 1e-12 * (1 + std::fabs(f)));
    // a multiplier of the first initial-state row reaches only x_0's stationarity
    sol[3 * nx] = 7.0;
    CHECK(mpcg::kkt_problem(r, model, N, init, c, sol.data()).stat >= 7.0);
    // z_U of the last variable (the last acceleration): stationarity and complementarity
    sol[3 * nx - 1] = 1e3;
    o = mpcg::kkt_problem(r, model, N, init, c, sol.data());
    CHECK(o.stat >= 900.0 && o.comp >= 1e3 * (1 - std::fabs(x[nx - 1])) * 0.999);
    r[MPCG_PP_DT] = 0.0;  // an invalid row
    o = mpcg::kkt_problem(r, model, N, init, c, sol.data());
    CHECK(o.stat != o.stat && o.prim != o.prim && o.comp != o.comp && o.f != o.f);
}

int main() {
    for (int model = 0; model < 2; ++model)
        for (int N : {2, 3, 20, 64, 65, 128}) one(N, model);
    if (fails) return 1;
    std::puts("ok");
    return 0;
}
