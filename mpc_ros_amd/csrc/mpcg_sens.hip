// mpc_ros_amd/csrc/mpcg_sens.hip -- k_sens: the feedback gains (mpcg_sens.h) of B solution records
// on CDNA4, and k_sens_apply, the correction u = clip(u0 + G [dstate; dcoeffs]).
//
// k_sens: one problem per wavefront.  The work area of sens_problem -- the stage data, the gains
// of every stage and the sweep's temporaries, sens_work_elems(N) doubles -- is the workgroup's
// dynamic LDS, sized by N at launch (11 KB at N = 20, 51 KB at N = 128: no HBM scratch at any
// horizon the solver accepts).  Stage data: lane k evaluates stage k (and 64 + k for N > 64)
// straight from the record, which is stored by variable, so the 64 lanes of a load read
// consecutive doubles.  The backward sweep holds the 8 x 8 cost-to-go one entry per lane; its
// phases exchange through LDS and are ordered by wave barriers (LDS instructions of one wavefront
// execute in issue order).  No solver state, no workspace, no atomics, no allocation: capturable.
// Nothing traps: a bad row or record ends in info 2 and NaN.
#include <hip/hip_runtime.h>

#include "mpcg_internal.h"
#include "mpcg_sens.h"
#include "wave_dev.h"

namespace mpcg {

// the kernel's executor: lane t runs job t, a wave barrier orders the phases
struct SensWaveLanes {
    int t;
    DevWave wv;
    template <class F>
    __device__ __forceinline__ void each(F&& f) {
        f(t);
        wv.sync();
    }
    template <class F>
    __device__ __forceinline__ bool any(F&& f) {
        const bool r = wv.any(f(t));
        wv.sync();
        return r;
    }
};

template <int MODEL>
__global__ void __launch_bounds__(64) k_sens(int64_t B, int N, PPRow hrow, double cvt, double brf,
                                             const double* __restrict__ rows, const double* __restrict__ coeffs,
                                             const double* __restrict__ sol, double* __restrict__ gain,
                                             double* __restrict__ dx, int32_t* __restrict__ info) {
    const int64_t p = blockIdx.x;
    if (p >= B) return;
    SensWaveLanes ex;
    ex.t = threadIdx.x;
    ex.wv.t = threadIdx.x;
    PPRow row = hrow;
    if (rows) {
#pragma unroll
        for (int j = 0; j < MPCG_PP_FIELDS; ++j) row.f[j] = rows[p * MPCG_PP_FIELDS + j];
    }
    double c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = coeffs[p * 4 + j];
    const int e = sens_problem(ex, mpcg_dyn_lds, row.f, MODEL, N, cvt, brf, c, sol + p * solution_elems(N),
                               gain + p * 2 * SENS_COLS, dx ? dx + p * (int64_t)SENS_COLS * (8 * N - 2) : nullptr);
    if (info && ex.t == 0) info[p] = e;
}

hipError_t launch_sens(int64_t B, int N, int model, const PPRow& row, double cvt, double brf, const double* rows,
                       const double* coeffs, const double* sol, double* gain, double* dx, int32_t* info,
                       hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (N < 2 || N > 128 || (model != 0 && model != 1)) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)sens_work_elems(N);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    if (model == 1)
        hipLaunchKernelGGL(k_sens<1>, dim3((unsigned)B), dim3(64), lds, stream, B, N, row, cvt, brf, rows, coeffs, sol,
                           gain, dx, info);
    else
        hipLaunchKernelGGL(k_sens<0>, dim3((unsigned)B), dim3(64), lds, stream, B, N, row, cvt, brf, rows, coeffs, sol,
                           gain, dx, info);
    return hipGetLastError();
}

// one robot per lane
__global__ void __launch_bounds__(256) k_sens_apply(int64_t B, PPRow hrow, const double* __restrict__ rows,
                                                    const double* __restrict__ gain, const double* __restrict__ u0,
                                                    const double* __restrict__ dstate,
                                                    const double* __restrict__ dcoeffs, double* __restrict__ u) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    double lim[MPCG_PP_FIELDS] = {};
    lim[MPCG_PP_ANGVEL] = rows ? rows[p * MPCG_PP_FIELDS + MPCG_PP_ANGVEL] : hrow.f[MPCG_PP_ANGVEL];
    lim[MPCG_PP_MAXTHR] = rows ? rows[p * MPCG_PP_FIELDS + MPCG_PP_MAXTHR] : hrow.f[MPCG_PP_MAXTHR];
    double g[2 * SENS_COLS], a[2], ds[6], dc[4], o[2];
#pragma unroll
    for (int j = 0; j < 2 * SENS_COLS; ++j) g[j] = gain[p * 2 * SENS_COLS + j];
#pragma unroll
    for (int j = 0; j < 6; ++j) ds[j] = dstate[p * 6 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) dc[j] = dcoeffs ? dcoeffs[p * 4 + j] : 0.0;
    a[0] = u0[p * 2];
    a[1] = u0[p * 2 + 1];
    sens_apply(lim, g, a, ds, dcoeffs ? dc : nullptr, o);
    u[p * 2] = o[0];
    u[p * 2 + 1] = o[1];
}

hipError_t launch_sens_apply(int64_t B, const PPRow& row, const double* rows, const double* gain, const double* u0,
                             const double* dstate, const double* dcoeffs, double* u, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sens_apply, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, row, rows, gain, u0,
                       dstate, dcoeffs, u);
    return hipGetLastError();
}

}  // namespace mpcg
