// mpc_ros_amd/csrc/mpcg_sens.h -- the first-order feedback law around a solution record
// (include/mpcg.h "Sensitivities of the solution"): G = d(omega_0, a_0) / d(state, coeffs) and the
// full primal columns dx, from the NLP and the record alone.  Like the certificate (mpcg_kkt.h) it
// shares no code with the solver (wide_core.h): the dynamics' first and second derivatives are
// written out again here from FG_eval's formulas.
//
// The system:  [ W + Sigma  J^T ] [ dx ]   [ a_c ]     W = Hessian of f + sum lambda_i g_i,
//              [ J          0   ] [ dl ] = [ b_c ]     Sigma = diag(zl / slack_l + zu / slack_u)
// is the optimality system of an equality-constrained LQ problem over the stages: minimise
// 1/2 dx^T (W + Sigma) dx - a^T dx subject to ds_0 = b_0, ds_{k+1} = A_k ds_k + B_k du_k + b_{k+1}.
// The rate terms couple u_k with u_{k-1}, so the recursion runs on the state augmented with the
// previous control, z_k = (s_k, u_{k-1}) (8 numbers; DESIGN.md "Linear algebra"):
//   backward  F = Qbar_k + T_k^T P_{k+1} T_k  (10 x 10 over (z, u); T = [Abar Bbar], 8 x 10),
//             Fuu = L L^T (2 x 2; not positive definite: info 1), w_i = L^-1 Fzu[i],
//             P_k = Fzz - w w^T, K_k = -Fuu^-1 Fuz; per coefficient column an affine term:
//             h = P_{k+1} dbar + p_{k+1}, f = g + T^T h, p_k = fz - w (L^-1 fu), kff = -Fuu^-1 fu;
//   forward   z_0 = (b_0, 0), u_k = K_k z_k + kff_k, z_{k+1} = T_k (z_k, u_k) + dbar_k.
//
// One body, sens_problem, host and device.  It is written as phases of independent jobs handed
// to an executor: the kernel (mpcg_sens.hip k_sens) runs one job per lane and orders the phases by
// wave barriers on its LDS work area; the host entry (mpcg_sens: no GPU, no handle) runs the 64
// "lanes" in a loop on a heap work area.  Stage data: one stage per lane (lanes loop for N > 64);
// the 8 x 8 cost-to-go: one entry per lane.  Evaluated without FMA contraction, in the same order
// on both sides: host and device differ by the platform's sin / cos only.
#ifndef MPCG_SENS_H
#define MPCG_SENS_H

#include "mpcg_pp.h"

namespace mpcg {

constexpr int SENS_COLS = MPCG_SENS_COLS;
constexpr int SENS_SD = 24;  // stage data per stage (sens_stage)
constexpr int SENS_GK = 24;  // gains per stage: K [2][8] | kff [2][4]
// offsets of the sweep's temporaries behind the per-stage arrays
constexpr int SENS_P = 0, SENS_PV = 64, SENS_T = 96, SENS_DG = 176, SENS_Y = 184, SENS_H = 264, SENS_F = 296,
              SENS_FV = 396, SENS_TMP = 440;
// doubles of one problem's work area (LDS on the device: 51 KB at N = 128)
MPCG_HD int sens_work_elems(int N) { return (SENS_SD + SENS_GK) * N + SENS_TMP; }

MPCG_HD bool sens_finite(double v) { return fabs(v) < INFINITY; }

// Stage k of the record sol -> sd[SENS_SD]:
//   0..7   A's entries: (0,2) (0,3) (1,2) (1,3) (2,3)=(5,3) (4,0) (4,3) (4,5)
//   8, 9   B's entries: (2,0)=(5,0), (3,1)
//   10..17 diag(W + Sigma) of x y theta v cte etheta omega a, without the rate terms
//   18..20 W (theta, v), (v, etheta), (v, omega)
//   21, 22 x_k and the multiplier of the cte row into stage k + 1 (the coefficient columns)
// r: the problem's parameter row, valid.  cvt, brf: constr_viol_tol and bound_relax_factor (the
// solver's bound relaxation).  false: a non-finite entry or a slack <= 0.
MPCG_HD bool sens_stage(const double* r, int model, int N, int k, const double* c, double cvt, double brf,
                        const double* sol, double* sd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int nx = 8 * N - 2;
    const double *x = sol, *zl = sol + nx, *zu = sol + 2 * nx, *lam = sol + 3 * nx;
    const bool last = k == N - 1;
    bool ok = true;
    double s[6], u[2] = {0.0, 0.0}, sig[8], ln[6];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sig[j] = 0.0;
        if (j < 6 || !last) {
            const int e = j < 6 ? j * N + k : 6 * N + (j - 6) * (N - 1) + k;
            const double hi = j < 6 ? r[MPCG_PP_BOUND] : (j == 6 ? r[MPCG_PP_ANGVEL] : r[MPCG_PP_MAXTHR]);
            const double rl = fmin(cvt, brf * fmax(1.0, hi));
            const double v = x[e], a = zl[e], b = zu[e];
            const double dl = v - (-hi - rl), du = (hi + rl) - v;
            ok = ok & sens_finite(v) & sens_finite(a) & sens_finite(b) & (dl > 0) & (du > 0);
            sig[j] = a / dl + b / du;
            if (j < 6) s[j] = v;
            else u[j - 6] = v;
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        ok = ok & sens_finite(lam[j * N + k]);
        ln[j] = last ? 0.0 : lam[j * N + k + 1];
    }
#pragma unroll
    for (int j = 0; j < SENS_SD; ++j) sd[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) sd[10 + j] = sig[j];
    sd[13] += 2.0 * r[MPCG_PP_W_V];
    sd[14] += 2.0 * r[MPCG_PP_W_CTE];
    sd[15] += 2.0 * r[MPCG_PP_W_EPSI];
    if (!last) {
        const double dt = r[MPCG_PP_DT], lf = r[MPCG_PP_LF];
        const double x0 = s[0], th = s[2], v = s[3], eth = s[5];
        const double sth = sin(th), cth = cos(th), se = sin(eth), ce = cos(eth);
        sd[0] = -(v * sth * dt);
        sd[1] = cth * dt;
        sd[2] = v * cth * dt;
        sd[3] = sth * dt;
        sd[4] = model == 1 ? u[0] / lf * dt : 0.0;
        sd[5] = c[1] + 2.0 * c[2] * x0 + 3.0 * c[3] * x0 * x0;
        sd[6] = se * dt;
        sd[7] = v * ce * dt;
        sd[8] = model == 1 ? v / lf * dt : dt;
        sd[9] = dt;
        // - sum_j ln[j] Hessian(F_j): the rows of stage k + 1 are s_{k+1} - F(s_k, u_k)
        sd[10] += -(ln[4] * (2.0 * c[2] + 6.0 * c[3] * x0));
        sd[12] += v * dt * (ln[0] * cth + ln[1] * sth);
        sd[15] += ln[4] * v * se * dt;
        sd[16] = sig[6] + 2.0 * r[MPCG_PP_W_ANGVEL];
        sd[17] = sig[7] + 2.0 * r[MPCG_PP_W_A];
        sd[18] = dt * (ln[0] * sth - ln[1] * cth);
        sd[19] = -(ln[4] * ce * dt);
        sd[20] = model == 1 ? -((ln[2] + ln[5]) * dt / lf) : 0.0;
        sd[21] = x0;
        sd[22] = ln[4];
    }
    return ok;
}

// T = [Abar Bbar] (8 x 10): z_{k+1} = T (z_k, u_k) + dbar, entry (m, b)
MPCG_HD double sens_T(const double* sd, int m, int b) {
    switch (m * 10 + b) {
        case 0: case 11: case 22: case 33: case 55: case 68: case 79: return 1.0;
        case 2: return sd[0];
        case 3: return sd[1];
        case 12: return sd[2];
        case 13: return sd[3];
        case 23: case 53: return sd[4];
        case 40: return sd[5];
        case 41: return -1.0;
        case 43: return sd[6];
        case 45: return sd[7];
        case 28: case 58: return sd[8];
        case 39: return sd[9];
        default: return 0.0;
    }
}

// Qbar (10 x 10 over (s, previous u, u)), entry (a, b) with a <= b; d0, d1: the rate weights
// 2 W_DANGVEL, 2 W_DA of the pair (k - 1, k), 0 at k = 0
MPCG_HD double sens_Q(const double* sd, double d0, double d1, int a, int b) {
    if (a == b) return a < 6 ? sd[10 + a] : a == 6 ? d0 : a == 7 ? d1 : a == 8 ? sd[16] + d0 : sd[17] + d1;
    switch (a * 10 + b) {
        case 23: return sd[18];
        case 35: return sd[19];
        case 38: return sd[20];
        case 68: return -d0;
        case 79: return -d1;
        default: return 0.0;
    }
}

// x^i and i x^(i-1), i = 0 .. 3
MPCG_HD double sens_pow(double x, int i) { return i == 0 ? 1.0 : i == 1 ? x : i == 2 ? x * x : x * x * x; }
MPCG_HD double sens_dpow(double x, int i) { return i == 0 ? 0.0 : i == 1 ? 1.0 : i == 2 ? 2.0 * x : 3.0 * x * x; }

// One problem.  ex: the executor -- each(f) runs f(t) for the 64 lanes t and orders it before what
// follows, any(f) is the OR of f(t).  w: sens_work_elems(N) doubles.  sol: the record; gain [2][10];
// dx [10][8N-2] or null.  Returns info (include/mpcg.h): 0, 1 (a stage's Fuu not positive
// definite), 2 (row, record or slack invalid); for 1 and 2 gain and dx are NaN.
template <class Ex>
MPCG_HD int sens_problem(Ex& ex, double* w, const double* r, int model, int N, double cvt, double brf,
                         const double* c, const double* sol, double* gain, double* dx) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int nx = 8 * N - 2;
    double* const SD = w;
    double* const GK = w + SENS_SD * N;
    double* const tmp = w + (SENS_SD + SENS_GK) * N;
    int info = 0;
    if (!pp_row_ok(r, model) || !(sens_finite(c[0]) & sens_finite(c[1]) & sens_finite(c[2]) & sens_finite(c[3])) ||
        !(cvt >= 0) || !(brf >= 0)) {
        info = 2;
    } else {
        // ---- stage data, one stage per lane
        const bool bad = ex.any([&](int t) {
            bool ok = true;
            for (int k = t; k < N; k += 64) ok = ok & sens_stage(r, model, N, k, c, cvt, brf, sol, SD + SENS_SD * k);
            return !ok;
        });
        if (bad) info = 2;
    }
    if (info == 0) {
        // ---- the backward sweep; terminal cost-to-go: the last stage's diagonal
        ex.each([&](int t) {
            const int i = t >> 3, j = t & 7;
            tmp[SENS_P + t] = (i == j && i < 6) ? SD[SENS_SD * (N - 1) + 10 + i] : 0.0;
            if (t < 32) tmp[SENS_PV + t] = 0.0;
        });
        for (int k = N - 2; k >= 0 && info == 0; --k) {
            const double* sd = SD + SENS_SD * k;
            double* gk = GK + SENS_GK * k;
            const double d0 = k >= 1 ? 2.0 * r[MPCG_PP_W_DANGVEL] : 0.0, d1 = k >= 1 ? 2.0 * r[MPCG_PP_W_DA] : 0.0;
            // T, and per coefficient column the defect x^i and the gradient term -i x^(i-1) lambda
            ex.each([&](int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                for (int j = t; j < 88; j += 64) {
                    if (j < 80) tmp[SENS_T + j] = sens_T(sd, j / 10, j % 10);
                    else if (j < 84) tmp[SENS_DG + j - 80] = sens_pow(sd[21], j - 80);
                    else tmp[SENS_DG + j - 80] = -(sens_dpow(sd[21], j - 84) * sd[22]);
                }
            });
            // Y = P T;  h = P dbar + p
            ex.each([&](int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                for (int j = t; j < 112; j += 64) {
                    if (j < 80) {
                        const int m = j / 10, b = j % 10;
                        double a = 0.0;
                        for (int n = 0; n < 8; ++n) a += tmp[SENS_P + m * 8 + n] * tmp[SENS_T + n * 10 + b];
                        tmp[SENS_Y + j] = a;
                    } else {
                        const int q = (j - 80) >> 3, m = (j - 80) & 7;
                        tmp[SENS_H + j - 80] = tmp[SENS_P + m * 8 + 4] * tmp[SENS_DG + q] + tmp[SENS_PV + q * 8 + m];
                    }
                }
            });
            // F = Qbar + T^T Y (the upper triangle, mirrored);  f = g + T^T h
            ex.each([&](int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                for (int j = t; j < 95; j += 64) {
                    if (j < 55) {
                        // entry j of the upper triangle, row by row: row a starts at 10 a - a (a - 1) / 2
                        const int a = (j >= 10) + (j >= 19) + (j >= 27) + (j >= 34) + (j >= 40) + (j >= 45) + (j >= 49) +
                                      (j >= 52) + (j >= 54);
                        const int b = j - (10 * a - a * (a - 1) / 2) + a;
                        double f = sens_Q(sd, d0, d1, a, b);
                        for (int m = 0; m < 8; ++m) f += tmp[SENS_T + m * 10 + a] * tmp[SENS_Y + m * 10 + b];
                        tmp[SENS_F + a * 10 + b] = f;
                        tmp[SENS_F + b * 10 + a] = f;
                    } else {
                        const int q = (j - 55) / 10, a = (j - 55) % 10;
                        double f = a == 0 ? tmp[SENS_DG + 4 + q] : 0.0;
                        for (int m = 0; m < 8; ++m) f += tmp[SENS_T + m * 10 + a] * tmp[SENS_H + q * 8 + m];
                        tmp[SENS_FV + j - 55] = f;
                    }
                }
            });
            // Fuu = L L^T (every lane the same bits)
            const double f00 = tmp[SENS_F + 88], f01 = tmp[SENS_F + 89], f11 = tmp[SENS_F + 99];
            if (!(f00 > 0) || !sens_finite(f00)) {
                info = 1;
                break;
            }
            const double l00 = sqrt(f00), l10 = f01 / l00, s11 = f11 - l10 * l10;
            if (!(s11 > 0) || !sens_finite(s11)) {
                info = 1;
                break;
            }
            const double l11 = sqrt(s11);
            // P = Fzz - w w^T, p = fz - w wf, K = -L^-T w, kff = -L^-T wf
            ex.each([&](int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                for (int j = t; j < 108; j += 64) {
                    // the row i of Fzu (j < 64: P's entry (i, i2); < 96: p's; < 104: K's column; else kff's)
                    const int i = j < 64 ? j >> 3 : j < 96 ? (j - 64) & 7 : j < 104 ? j - 96 : -1;
                    const int q = j < 64 ? -1 : j < 96 ? (j - 64) >> 3 : j < 104 ? -1 : j - 104;
                    double wi0 = 0.0, wi1 = 0.0, wq0 = 0.0, wq1 = 0.0;
                    if (i >= 0) {
                        wi0 = tmp[SENS_F + i * 10 + 8] / l00;
                        wi1 = (tmp[SENS_F + i * 10 + 9] - l10 * wi0) / l11;
                    }
                    if (q >= 0) {
                        wq0 = tmp[SENS_FV + q * 10 + 8] / l00;
                        wq1 = (tmp[SENS_FV + q * 10 + 9] - l10 * wq0) / l11;
                    }
                    if (j < 64) {
                        const int i2 = j & 7;
                        const double v0 = tmp[SENS_F + i2 * 10 + 8] / l00;
                        const double v1 = (tmp[SENS_F + i2 * 10 + 9] - l10 * v0) / l11;
                        tmp[SENS_P + j] = tmp[SENS_F + i * 10 + i2] - (wi0 * v0 + wi1 * v1);
                    } else if (j < 96) {
                        tmp[SENS_PV + q * 8 + i] = tmp[SENS_FV + q * 10 + i] - (wi0 * wq0 + wi1 * wq1);
                    } else if (j < 104) {
                        const double y1 = wi1 / l11, y0 = (wi0 - l10 * y1) / l00;
                        gk[i] = -y0;
                        gk[8 + i] = -y1;
                    } else {
                        const double y1 = wq1 / l11, y0 = (wq0 - l10 * y1) / l00;
                        gk[16 + q] = -y0;
                        gk[20 + q] = -y1;
                    }
                }
            });
        }
    }
    if (info == 0) {
        // ---- the forward sweep: one column per lane (the gain needs stage 0 only)
        ex.each([&](int t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
            if (t >= SENS_COLS) return;
            const int q = t - 6;
            double z[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (t < 6) z[t] = 1.0;
            double* col = dx ? dx + (size_t)t * nx : nullptr;
            for (int k = 0; k < N - 1; ++k) {
                const double* sd = SD + SENS_SD * k;
                const double* gk = GK + SENS_GK * k;
                double u0 = q >= 0 ? gk[16 + q] : 0.0, u1 = q >= 0 ? gk[20 + q] : 0.0;
                for (int j = 0; j < 8; ++j) {
                    u0 += gk[j] * z[j];
                    u1 += gk[8 + j] * z[j];
                }
                if (k == 0) {
                    gain[t] = u0;
                    gain[SENS_COLS + t] = u1;
                }
                if (!col) break;
                for (int j = 0; j < 6; ++j) col[j * N + k] = z[j];
                col[6 * N + k] = u0;
                col[7 * N - 1 + k] = u1;
                const double turn = sd[4] * z[3] + sd[8] * u0;
                const double n0 = z[0] + sd[0] * z[2] + sd[1] * z[3];
                const double n1 = z[1] + sd[2] * z[2] + sd[3] * z[3];
                const double n4 = sd[5] * z[0] - z[1] + sd[6] * z[3] + sd[7] * z[5] + (q >= 0 ? sens_pow(sd[21], q) : 0.0);
                z[0] = n0;
                z[1] = n1;
                z[2] = z[2] + turn;
                z[5] = z[5] + turn;
                z[3] = z[3] + sd[9] * u1;
                z[4] = n4;
                z[6] = u0;
                z[7] = u1;
            }
            if (col)
                for (int j = 0; j < 6; ++j) col[j * N + N - 1] = z[j];
        });
    } else {
        ex.each([&](int t) {
            const double nan = __builtin_nan("");
            if (t < 2 * SENS_COLS) gain[t] = nan;
            if (dx)
                for (int j = t; j < SENS_COLS * nx; j += 64) dx[j] = nan;
        });
    }
    return info;
}

// the host's executor: the 64 lanes in a loop
struct SensHostLanes {
    template <class F>
    void each(F&& f) {
        for (int t = 0; t < 64; ++t) f(t);
    }
    template <class F>
    bool any(F&& f) {
        bool r = false;
        for (int t = 0; t < 64; ++t) r = f(t) || r;
        return r;
    }
};

// mpcg_sens_apply_device's rule for one robot: u = clip(u0 + gain [dstate; dcoeffs]) to +-ANGVEL,
// +-MAXTHR of the row r; dcoeffs null = 0; a sum that is not finite (a NaN gain) gives u0
MPCG_HD void sens_apply(const double* r, const double* gain, const double* u0, const double* dstate,
                        const double* dcoeffs, double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double hi = i == 0 ? r[MPCG_PP_ANGVEL] : r[MPCG_PP_MAXTHR];
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) a += gain[i * SENS_COLS + j] * dstate[j];
        if (dcoeffs) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a += gain[i * SENS_COLS + 6 + j] * dcoeffs[j];
        }
        const double v = u0[i] + a;
        u[i] = !sens_finite(v) ? u0[i] : v > hi ? hi : v < -hi ? -hi : v;
    }
}

}  // namespace mpcg
#endif
