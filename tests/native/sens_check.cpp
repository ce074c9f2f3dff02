// tests/native/sens_check.cpp -- TEST HARNESS ONLY.
//
// A stand-alone program over mpc_ros_amd/csrc/mpcg_sens.h (the feedback gains' stage body, its
// sweeps and the host executor), built with -fsanitize=address,undefined and run directly by
// tests/test_sens_host.py on solution records: every index the sweeps form (the record's four
// parts, the per-stage arrays of the work area, the columns of dx) lands in exactly sized heap
// arrays, so an index past one of them is an ASan report.
//
// stdin:  model N B constr_viol_tol bound_relax_factor, the parameter row (16 doubles), then per
//         problem the 4 coefficients and the record (3 (8N - 2) + 6N doubles).
// stdout: per problem one line: info, the 20 gain entries, the 10 (8N - 2) entries of dx.
// Then the correction rule on the first problem's gain (one line: u with dcoeffs, u without).
#include <cmath>
#include <cstdio>
#include <vector>

#include "mpcg_sens.h"

int main() {
    int model = 0, N = 0, B = 0;
    double cvt = 0, brf = 0, r[MPCG_PP_FIELDS];
    if (std::scanf("%d %d %d %lf %lf", &model, &N, &B, &cvt, &brf) != 5 || N < 2 || N > 128 || B < 1) return 2;
    for (double& v : r)
        if (std::scanf("%lf", &v) != 1) return 2;
    const int nx = 8 * N - 2, ne = 3 * nx + 6 * N;
    std::vector<double> first_gain;
    for (int b = 0; b < B; ++b) {
        std::vector<double> c(4), sol((size_t)ne), w((size_t)mpcg::sens_work_elems(N)), gain(2 * mpcg::SENS_COLS),
            dx((size_t)mpcg::SENS_COLS * nx);
        for (double& v : c)
            if (std::scanf("%lf", &v) != 1) return 2;
        for (double& v : sol)
            if (std::scanf("%lf", &v) != 1) return 2;
        mpcg::SensHostLanes ex;
        const int info = mpcg::sens_problem(ex, w.data(), r, model, N, cvt, brf, c.data(), sol.data(), gain.data(),
                                            dx.data());
        // without dx: the same gain
        std::vector<double> g2(2 * mpcg::SENS_COLS);
        const int info2 =
            mpcg::sens_problem(ex, w.data(), r, model, N, cvt, brf, c.data(), sol.data(), g2.data(), nullptr);
        if (info2 != info) return 3;
        for (int j = 0; j < 2 * mpcg::SENS_COLS; ++j)
            if (!(g2[j] == gain[j]) && !(g2[j] != g2[j] && gain[j] != gain[j])) return 3;
        std::printf("%d", info);
        for (double v : gain) std::printf(" %.17g", v);
        for (double v : dx) std::printf(" %.17g", v);
        std::printf("\n");
        if (b == 0) first_gain = gain;
    }
    const double u0[2] = {0.25, -0.5}, ds[6] = {0.01, -0.02, 0.03, 0.04, -0.05, 0.06}, dc[4] = {0.1, -0.1, 0.05, 0.02};
    double u[2], v[2];
    mpcg::sens_apply(r, first_gain.data(), u0, ds, dc, u);
    mpcg::sens_apply(r, first_gain.data(), u0, ds, nullptr, v);
    std::printf("%.17g %.17g %.17g %.17g\n", u[0], u[1], v[0], v[1]);
    return 0;
}
