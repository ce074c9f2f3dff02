// mpc_ros_amd/csrc/mpcg_kkt.h -- the KKT certificate of a solution record (include/mpcg.h
// MPCG_SOL_*): the first-order conditions of the reference NLP (FG_eval, mpc_planner.cpp:102-217,
// with MPC::Solve's ORIGINAL bounds, :281-348) evaluated at a given (x, z_L, z_U, lambda) from
// the NLP alone.  It shares no code with the solver (wide_core.h): the dynamics, their
// derivatives and the cost are written out again here from FG_eval's formulas, so an error in the
// solver's model, scaling or sign conventions cannot cancel in its own certificate.
//
// One stage body, kkt_stage, host and device: the kernel (mpcg_kkt.hip k_kkt_certify) calls it
// per lane (lane k = stage k, the neighbours' values by lane shifts), the host entry kkt_problem
// calls it in a loop (mpcg_kkt: no GPU, no handle).  Evaluated without FMA contraction; host and
// device still agree only to rounding, not bitwise: sin / cos are the platform's (a few ulp apart)
// and the objective is summed by a tree on the device and in stage order on the host.
//
// Convention (Ipopt / CppAD): L = f + sum lambda_i g_i, stationarity grad f + J^T lambda - z_L + z_U = 0.
// Row s N + k (s: x y theta v cte etheta): k = 0 the initial-state row g = var, bound state[s];
// k >= 1 the defect var_k - F_s(stage k - 1), bound 0.
#ifndef MPCG_KKT_H
#define MPCG_KKT_H

#include "mpcg_pp.h"

namespace mpcg {

// the certificate of one problem, or one stage's share of it: cert[4]
struct KktCert {
    double stat;  // max |grad f + J^T lambda - z_L + z_U|
    double prim;  // max(|g - g_bound|, bound violation of x)
    double comp;  // max(|(x - x_L) z_L|, |(x_U - x) z_U|)
    double f;     // objective
};

// max that keeps a NaN (a certificate must not lose one in a reduction)
MPCG_HD double kkt_max(double a, double b) { return (b > a || b != b) ? b : a; }
MPCG_HD KktCert kkt_join(const KktCert& a, const KktCert& b) {
    return KktCert{kkt_max(a.stat, b.stat), kkt_max(a.prim, b.prim), kkt_max(a.comp, b.comp), a.f + b.f};
}
MPCG_HD KktCert kkt_nan() {
    const double n = __builtin_nan("");
    return KktCert{n, n, n, n};
}

// One step of the model, F[6] = the stage that follows (sp, up) with zero defect: the right-hand
// sides of FG_eval's dynamics rows (diff-drive, or model 1 the bicycle), as the rows below subtract
// them.  Also the terminal stage of a shifted record (mpcg_shift.h).
MPCG_HD void kkt_step(const double* r, int model, const double* c, const double* sp, const double* up, double* F) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dt = r[MPCG_PP_DT], lf = r[MPCG_PP_LF];
    const double x0 = sp[0], y0 = sp[1], th0 = sp[2], v0 = sp[3], eth0 = sp[5];
    const double turn = model == 1 ? v0 * up[0] / lf * dt : up[0] * dt;
    double fx = 0.0, pw = 1.0;  // f(x0) = sum c_k x0^k, the powers by repeated multiplication
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        fx += c[q] * pw;
        pw *= x0;
    }
    F[0] = x0 + v0 * cos(th0) * dt;
    F[1] = y0 + v0 * sin(th0) * dt;
    F[2] = th0 + turn;
    F[3] = v0 + up[1] * dt;
    F[4] = (fx - y0) + v0 * sin(eth0) * dt;
    F[5] = eth0 + turn;
}

// One stage.  r: the problem's parameter row (MPCG_PP_*), valid.  c[4], init[6]: the problem.
// Own values: s[6] u[2] (u read for k < N - 1), zl[8] zu[8] (6 for the last stage), lam[6] the
// multipliers of the rows into stage k.  Neighbours: sp[6] up[2] of stage k - 1 (read for k >= 1),
// ln[6] the multipliers of the rows into stage k + 1 and un[2] the controls of stage k + 1 (ln read
// for k < N - 1, un for k <= N - 3).
MPCG_HD KktCert kkt_stage(const double* r, int model, int N, int k, const double* c, const double* init,
                          const double* s, const double* u, const double* zl, const double* zu, const double* lam,
                          const double* sp, const double* up, const double* ln, const double* un) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dt = r[MPCG_PP_DT], lf = r[MPCG_PP_LF];
    const bool last = k == N - 1;
    KktCert o{0.0, 0.0, 0.0, 0.0};
    // ---- the rows into stage k
    double g[6];
    if (k == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) g[j] = s[j] - init[j];
    } else {
        double F[6];
        kkt_step(r, model, c, sp, up, F);
#pragma unroll
        for (int j = 0; j < 6; ++j) g[j] = s[j] - F[j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) o.prim = kkt_max(o.prim, fabs(g[j]));
    // ---- grad f + J^T lambda of the stage's variables
    double d[8];
    d[0] = lam[0];
    d[1] = lam[1];
    d[2] = lam[2];
    d[3] = 2.0 * r[MPCG_PP_W_V] * (s[3] - r[MPCG_PP_REF_V]) + lam[3];
    d[4] = 2.0 * r[MPCG_PP_W_CTE] * (s[4] - r[MPCG_PP_REF_CTE]) + lam[4];
    d[5] = 2.0 * r[MPCG_PP_W_EPSI] * (s[5] - r[MPCG_PP_REF_ETHETA]) + lam[5];
    d[6] = 0.0;
    d[7] = 0.0;
    double e1 = s[4] - r[MPCG_PP_REF_CTE], e2 = s[5] - r[MPCG_PP_REF_ETHETA], e3 = s[3] - r[MPCG_PP_REF_V];
    o.f = r[MPCG_PP_W_CTE] * e1 * e1 + r[MPCG_PP_W_EPSI] * e2 * e2 + r[MPCG_PP_W_V] * e3 * e3;
    if (!last) {
        const double x0 = s[0], th0 = s[2], v0 = s[3], eth0 = s[5];
        const double sth = sin(th0), cth = cos(th0), se = sin(eth0), ce = cos(eth0);
        const double f1 = c[1] + 2.0 * c[2] * x0 + 3.0 * c[3] * x0 * x0;
        const double tw = model == 1 ? v0 / lf * dt : dt;        // d(turn)/d(w)
        const double tv = model == 1 ? u[0] / lf * dt : 0.0;     // d(turn)/d(v)
        const double lh = ln[2] + ln[5];
        // (the rows of stage k + 1 in the columns of stage k: -dF/d(s, u))
        d[0] += -ln[0] - f1 * ln[4];
        d[1] += -ln[1] + ln[4];
        d[2] += v0 * sth * dt * ln[0] - v0 * cth * dt * ln[1] - ln[2];
        d[3] += -cth * dt * ln[0] - sth * dt * ln[1] - ln[3] - se * dt * ln[4] - tv * lh;
        d[5] += -v0 * ce * dt * ln[4] - ln[5];
        d[6] = 2.0 * r[MPCG_PP_W_ANGVEL] * u[0] - tw * lh;
        d[7] = 2.0 * r[MPCG_PP_W_A] * u[1] - dt * ln[3];
        o.f += r[MPCG_PP_W_ANGVEL] * u[0] * u[0] + r[MPCG_PP_W_A] * u[1] * u[1];
        if (k >= 1) {
            d[6] += 2.0 * r[MPCG_PP_W_DANGVEL] * (u[0] - up[0]);
            d[7] += 2.0 * r[MPCG_PP_W_DA] * (u[1] - up[1]);
        }
        if (k <= N - 3) {
            const double dw = un[0] - u[0], da = un[1] - u[1];
            d[6] -= 2.0 * r[MPCG_PP_W_DANGVEL] * dw;
            d[7] -= 2.0 * r[MPCG_PP_W_DA] * da;
            o.f += r[MPCG_PP_W_DANGVEL] * dw * dw + r[MPCG_PP_W_DA] * da * da;
        }
    }
    // ---- stationarity, bounds and complementarity, against MPC::Solve's own bounds
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < 6 || !last) {
            const double x = j < 6 ? s[j] : u[j - 6];
            const double hi = j < 6 ? r[MPCG_PP_BOUND] : (j == 6 ? r[MPCG_PP_ANGVEL] : r[MPCG_PP_MAXTHR]);
            const double lo = -hi;
            o.stat = kkt_max(o.stat, fabs(d[j] - zl[j] + zu[j]));
            o.prim = kkt_max(o.prim, kkt_max(lo - x, x - hi));
            o.comp = kkt_max(o.comp, kkt_max(fabs((x - lo) * zl[j]), fabs((hi - x) * zu[j])));
        }
    }
    return o;
}

// One problem on the host: the stage body over k = 0 .. N - 1 on the record sol (x | z_L | z_U |
// lambda, solution_elems(N) doubles), the objective summed in stage order.  An invalid row: NaN.
inline KktCert kkt_problem(const double* r, int model, int N, const double* init, const double* c, const double* sol) {
    if (!pp_row_ok(r, model)) return kkt_nan();
    const int nx = 8 * N - 2;
    const double *x = sol, *zl = sol + nx, *zu = sol + 2 * nx, *lam = sol + 3 * nx;
    KktCert o{0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < N; ++k) {
        double s[6], u[2] = {0, 0}, a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l[6];
        double sp[6] = {0, 0, 0, 0, 0, 0}, up[2] = {0, 0}, ln[6] = {0, 0, 0, 0, 0, 0}, un[2] = {0, 0};
        for (int j = 0; j < 6; ++j) {
            s[j] = x[j * N + k];
            a[j] = zl[j * N + k];
            b[j] = zu[j * N + k];
            l[j] = lam[j * N + k];
            if (k >= 1) sp[j] = x[j * N + k - 1];
            if (k < N - 1) ln[j] = lam[j * N + k + 1];
        }
        for (int j = 0; j < 2; ++j) {
            const int base = 6 * N + j * (N - 1);
            if (k < N - 1) {
                u[j] = x[base + k];
                a[6 + j] = zl[base + k];
                b[6 + j] = zu[base + k];
            }
            if (k >= 1) up[j] = x[base + k - 1];
            if (k <= N - 3) un[j] = x[base + k + 1];
        }
        o = kkt_join(o, kkt_stage(r, model, N, k, c, init, s, u, a, b, l, sp, up, ln, un));
    }
    return o;
}

}  // namespace mpcg
#endif
