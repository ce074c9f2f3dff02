// mpc_ros_amd/csrc/mpcg_shift.hip -- k_shift_solution / k_shift_rollout: the shift rule
// (mpcg_shift.h) on B solution records on CDNA4.  One problem per wavefront.  The 64 lanes stride
// the record's elements, so every global read and write is a contiguous run of doubles, and every
// LDS write lands on consecutive banks.  The whole source record is staged in LDS (dynamic, 3 (8N -
// 2) + 6N + 6 doubles: 4.8 KB at N = 20, 30.7 KB at N = 128) before anything is written: the call
// in place is correct, and the (x, y) pairs and the terminal step read their operands without a
// second global pass.  The rotation's sin / cos and the terminal step are computed by every lane
// alike (one instruction stream per wavefront); the terminal state goes through six more LDS
// doubles, so no lane indexes a private array.  Whether a problem is shifted, copied or left alone
// is wave-uniform.
#include <hip/hip_runtime.h>

#include "mpcg_internal.h"
#include "mpcg_shift.h"

namespace mpcg {

// the shift of problem p by the wavefront: in -> out (may alias), through the LDS image rec
template <int MODEL>
__device__ __forceinline__ void shift_wave(double* rec, int N, const double* row, const double* state,
                                           const double* coeffs, const double* motion, const double* in, double* out) {
    const int t = threadIdx.x, ne = shift_record_elems(N);
    for (int e = t; e < ne; e += 64) rec[e] = in[e];
    __syncthreads();
    const ShiftFrame f = shift_frame(motion);
    double term[6];
    shift_terminal(rec, N, MODEL, row, coeffs, state, f, term);
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) rec[ne + j] = term[j];
    }
    __syncthreads();
    for (int e = t; e < ne; e += 64) out[e] = shift_elem(rec, N, e, f, state, rec + ne);
}

template <int MODEL>
__global__ void __launch_bounds__(64) k_shift_solution(int64_t B, int N, PPRow hrow, const double* __restrict__ rows,
                                                       const double* __restrict__ state,
                                                       const double* __restrict__ coeffs,
                                                       const double* __restrict__ motion,
                                                       const int32_t* __restrict__ mask, const double* in, double* out) {
    extern __shared__ double rec[];
    const int64_t p = blockIdx.x;
    if (p >= B) return;
    const int ne = shift_record_elems(N);
    const double* src = in + p * ne;
    double* dst = out + p * ne;
    if (mask && mask[p] == 0) {  // (wave-uniform) the record unchanged
        if (src != dst)
            for (int e = threadIdx.x; e < ne; e += 64) dst[e] = src[e];
        return;
    }
    PPRow row = hrow;
    if (rows) {
#pragma unroll
        for (int j = 0; j < MPCG_PP_FIELDS; ++j) row.f[j] = rows[p * MPCG_PP_FIELDS + j];
    }
    shift_wave<MODEL>(rec, N, row.f, state + p * 6, coeffs + p * 4, motion + p * 3, src, dst);
}

// The rollout's shift (mpcg_rollout_device_start), after the tick's preprocessing: robot p uses its
// record if carry_ok[p] != 0, done[p] == 0 and start_mode != COLD -- shifted in place by the motion
// from carry_pose[p] to pose[p], its mode start_mode; every other robot's mode is COLD.  mu0s[p] =
// mu0; carry_pose[p] takes the tick's pose of a running robot.
template <int MODEL>
__global__ void __launch_bounds__(64) k_shift_rollout(int64_t B, int N, int start_mode, double mu0,
                                                      const double* __restrict__ rows, const double* __restrict__ state,
                                                      const double* __restrict__ coeffs,
                                                      const double* __restrict__ pose, const int32_t* __restrict__ done,
                                                      const int32_t* __restrict__ carry_ok, double* carry_pose,
                                                      double* carry_sol, int32_t* __restrict__ modes,
                                                      double* __restrict__ mu0s) {
    extern __shared__ double rec[];
    const int64_t p = blockIdx.x;
    if (p >= B) return;
    const int t = threadIdx.x;
    const bool run = done[p] == 0, use = run && carry_ok[p] != 0 && start_mode != MPCG_START_COLD;  // (wave-uniform)
    double motion[3];
    shift_motion(carry_pose + p * 3, pose + p * 3, motion);
    __syncthreads();  // (every lane has read carry_pose)
    if (t == 0) {
        modes[p] = use ? start_mode : MPCG_START_COLD;
        mu0s[p] = mu0;
    }
    if (run && t < 3) carry_pose[p * 3 + t] = pose[p * 3 + t];
    if (!use) return;
    double* r = carry_sol + p * shift_record_elems(N);
    shift_wave<MODEL>(rec, N, rows + p * MPCG_PP_FIELDS, state + p * 6, coeffs + p * 4, motion, r, r);
}

// after the solve: carry_ok[p] = running and solved (status 1 or 4)
__global__ void __launch_bounds__(256) k_carry_flag(int64_t B, const int32_t* __restrict__ done,
                                                    const int32_t* __restrict__ status, int32_t* __restrict__ carry_ok) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    carry_ok[p] = done[p] == 0 && (status[p] == 1 || status[p] == 4) ? 1 : 0;
}

static size_t shift_lds_bytes(int N) { return sizeof(double) * (size_t)(shift_record_elems(N) + 6); }
static bool shift_args_ok(int N, int model) { return N >= 2 && N <= 128 && (model == 0 || model == 1); }

hipError_t launch_shift_solution(int64_t B, int N, int model, const PPRow& row, const double* rows, const double* state,
                                 const double* coeffs, const double* motion, const int32_t* mask, const double* in,
                                 double* out, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (!shift_args_ok(N, model)) return hipErrorInvalidValue;
    if (model == 1)
        hipLaunchKernelGGL(k_shift_solution<1>, dim3((unsigned)B), dim3(64), shift_lds_bytes(N), stream, B, N, row, rows,
                           state, coeffs, motion, mask, in, out);
    else
        hipLaunchKernelGGL(k_shift_solution<0>, dim3((unsigned)B), dim3(64), shift_lds_bytes(N), stream, B, N, row, rows,
                           state, coeffs, motion, mask, in, out);
    return hipGetLastError();
}

hipError_t launch_shift_rollout(int64_t B, int N, int model, int start_mode, double mu0, const double* rows,
                                const double* state, const double* coeffs, const double* pose, const int32_t* done,
                                const int32_t* carry_ok, double* carry_pose, double* carry_sol, int32_t* modes,
                                double* mu0s, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (!shift_args_ok(N, model)) return hipErrorInvalidValue;
    if (model == 1)
        hipLaunchKernelGGL(k_shift_rollout<1>, dim3((unsigned)B), dim3(64), shift_lds_bytes(N), stream, B, N, start_mode,
                           mu0, rows, state, coeffs, pose, done, carry_ok, carry_pose, carry_sol, modes, mu0s);
    else
        hipLaunchKernelGGL(k_shift_rollout<0>, dim3((unsigned)B), dim3(64), shift_lds_bytes(N), stream, B, N, start_mode,
                           mu0, rows, state, coeffs, pose, done, carry_ok, carry_pose, carry_sol, modes, mu0s);
    return hipGetLastError();
}

hipError_t launch_carry_flag(int64_t B, const int32_t* done, const int32_t* status, int32_t* carry_ok,
                             hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_carry_flag, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, done, status, carry_ok);
    return hipGetLastError();
}

}  // namespace mpcg
