// mpc_ros_amd/csrc/mpcg_kkt.hip -- k_kkt_certify: the KKT certificate (mpcg_kkt.h) of B solution
// records on CDNA4.  One problem per wavefront, lane k = stage k (a lane owns stages k and 64 + k
// for 64 < N <= 128, as the solver's two-block instances do).  A lane reads its stage's entries
// of the record straight into registers -- the record is stored by variable, x(N) | y(N) | ...,
// so the 64 lanes of a load read consecutive doubles -- and takes the neighbouring stages' values
// by the DPP lane shifts of wave_dev.h (wave_shr:1 / wave_shl:1; across the two blocks by a lane
// read).  The three maxima and the objective go through the solver's butterfly partners
// (DevWaveBase::rpart).  No LDS.
#include <hip/hip_runtime.h>

#include "mpcg_internal.h"
#include "mpcg_kkt.h"
#include "wave_dev.h"

namespace mpcg {

// the stage's own values
struct KktLane {
    double s[6], u[2], zl[8], zu[8], lam[6];
};

template <int MODEL>
__global__ void __launch_bounds__(64) k_kkt_certify(int64_t B, int N, PPRow hrow, const double* __restrict__ rows,
                                                    const double* __restrict__ state,
                                                    const double* __restrict__ coeffs,
                                                    const double* __restrict__ sol, double* __restrict__ cert) {
    const int64_t p = blockIdx.x;
    if (p >= B) return;
    const int t = threadIdx.x;
    DevWave wv;
    wv.t = t;
    PPRow row = hrow;
    if (rows) {
#pragma unroll
        for (int j = 0; j < MPCG_PP_FIELDS; ++j) row.f[j] = rows[p * MPCG_PP_FIELDS + j];
    }
    if (!pp_row_ok(row.f, MODEL)) {  // (wave-uniform)
        if (t < 4) cert[p * 4 + t] = __builtin_nan("");
        return;
    }
    double init[6], c[4];
#pragma unroll
    for (int j = 0; j < 6; ++j) init[j] = state[p * 6 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = coeffs[p * 4 + j];
    const int nx = 8 * N - 2;
    const double* x = sol + p * solution_elems(N);
    const double *zl = x + nx, *zu = x + 2 * nx, *lam = x + 3 * nx;
    const int nb = N > 64 ? 2 : 1;
    KktLane v[2];
    for (int b = 0; b < 2; ++b) {
        const int k = t + 64 * b;
        const bool act = b < nb && k < N, ctl = act && k < N - 1;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            v[b].s[j] = act ? x[j * N + k] : 0.0;
            v[b].zl[j] = act ? zl[j * N + k] : 0.0;
            v[b].zu[j] = act ? zu[j * N + k] : 0.0;
            v[b].lam[j] = act ? lam[j * N + k] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = 6 * N + j * (N - 1) + k;
            v[b].u[j] = ctl ? x[e] : 0.0;
            v[b].zl[6 + j] = ctl ? zl[e] : 0.0;
            v[b].zu[6 + j] = ctl ? zu[e] : 0.0;
        }
    }
    KktCert o{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b >= nb) break;  // (wave-uniform)
        const int k = t + 64 * b;
        // the neighbours: stage k - 1 from the lane below (lane 0 of the second block: lane 63 of
        // the first), stage k + 1 from the lane above (lane 63 of the first block: lane 0 of the second)
        double sp[6], up[2], ln[6], un[2];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            sp[j] = wv.up1(v[b].s[j]);
            ln[j] = wv.dn1(v[b].lam[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            up[j] = wv.up1(v[b].u[j]);
            un[j] = wv.dn1(v[b].u[j]);
        }
        if (nb == 2) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double s63 = wv.lane63(v[0].s[j]), l0 = wv.lane0(v[1].lam[j]);
                if (b == 1 && t == 0) sp[j] = s63;
                if (b == 0 && t == 63) ln[j] = l0;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double u63 = wv.lane63(v[0].u[j]), u0 = wv.lane0(v[1].u[j]);
                if (b == 1 && t == 0) up[j] = u63;
                if (b == 0 && t == 63) un[j] = u0;
            }
        }
        if (k < N)
            o = kkt_join(o, kkt_stage(row.f, MODEL, N, k, c, init, v[b].s, v[b].u, v[b].zl, v[b].zu, v[b].lam, sp, up,
                                      ln, un));
    }
    // the butterfly: every lane ends with the same bits
#define MPCG_KKT_STEP(s)                                                                                   \
    o = kkt_join(o, KktCert{wv.rpart<s>(o.stat), wv.rpart<s>(o.prim), wv.rpart<s>(o.comp), wv.rpart<s>(o.f)});
    MPCG_KKT_STEP(0)
    MPCG_KKT_STEP(1)
    MPCG_KKT_STEP(2)
    MPCG_KKT_STEP(3)
    MPCG_KKT_STEP(4)
    MPCG_KKT_STEP(5)
#undef MPCG_KKT_STEP
    if (t == 0) {
        cert[p * 4 + 0] = o.stat;
        cert[p * 4 + 1] = o.prim;
        cert[p * 4 + 2] = o.comp;
        cert[p * 4 + 3] = o.f;
    }
}

hipError_t launch_kkt_certify(int64_t B, int N, int model, const PPRow& row, const double* rows, const double* state,
                              const double* coeffs, const double* sol, double* cert, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (N < 2 || N > 128 || (model != 0 && model != 1)) return hipErrorInvalidValue;
    if (model == 1)
        hipLaunchKernelGGL(k_kkt_certify<1>, dim3((unsigned)B), dim3(64), 0, stream, B, N, row, rows, state, coeffs, sol,
                           cert);
    else
        hipLaunchKernelGGL(k_kkt_certify<0>, dim3((unsigned)B), dim3(64), 0, stream, B, N, row, rows, state, coeffs, sol,
                           cert);
    return hipGetLastError();
}

}  // namespace mpcg
