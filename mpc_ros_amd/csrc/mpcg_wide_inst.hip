// mpc_ros_amd/csrc/mpcg_wide_inst.hip -- the solver kernel instances, one group per
// translation unit: build.py compiles this file once per MPCG_INST value (0..33, in
// parallel) and links the objects into libmpcg.so.  The groups are listed with their
// instances in wide_plan.h (MPCG_WIDE_SOLVE_INSTANCES / _RESUME_ / _WARM_INSTANCES; groups 12..19:
// the per-problem instances, MPCG_WIDE_PP_SOLVE_INSTANCES / _PP_RESUME_INSTANCES; groups 20..33:
// the started solve's, MPCG_WIDE_START_INSTANCES / _START_RESUME_INSTANCES).
#include "mpcg_wide_kern.h"

#ifndef MPCG_INST
#error "compile with -DMPCG_INST=<group>"
#endif

namespace mpcg {

#define MPCG_DEF_SOLVE(g, M, S, T, NB, D, W)                                                  \
    template <>                                                                               \
    const void* solve_kernel_fn<M, S, T, NB, D, W>() {                                       \
        return (const void*)k_solve_wide<M, S, T, NB, D, W>;                                  \
    }
#define MPCG_DEF_WARM(g, M, S, T, NB, D, W)                                                   \
    template <>                                                                               \
    const void* warm_kernel_fn<M, S, T, NB, D, W>() {                                        \
        return (const void*)k_warm_wide<M, S, T, NB, D, W>;                                   \
    }
#define MPCG_DEF_RESUME(g, M, S, T, NB)                                                       \
    template <>                                                                               \
    const void* resume_kernel_fn<M, S, T, NB>() {                                            \
        return (const void*)k_resume_wide<M, S, T, NB>;                                       \
    }
#define MPCG_DEF_PP_SOLVE(g, M, S, T, NB, D, W)                                               \
    template <>                                                                               \
    const void* pp_solve_kernel_fn<M, S, T, NB, D, W>() {                                    \
        return (const void*)k_solve_wide_pp<M, S, T, NB, D, W>;                               \
    }
#define MPCG_DEF_PP_RESUME(g, M, S, T, NB)                                                    \
    template <>                                                                               \
    const void* pp_resume_kernel_fn<M, S, T, NB>() {                                         \
        return (const void*)k_resume_wide_pp<M, S, T, NB>;                                    \
    }
#define MPCG_DEF_START(g, M, S, T, NB, D, W)                                                  \
    template <>                                                                               \
    const void* start_kernel_fn<M, S, T, NB, D, W>() {                                       \
        return (const void*)k_start_wide<M, S, T, NB, D, W>;                                  \
    }
#define MPCG_DEF_START_RESUME(g, M, S, T, NB)                                                 \
    template <>                                                                               \
    const void* start_resume_kernel_fn<M, S, T, NB>() {                                      \
        return (const void*)k_resume_wide_start<M, S, T, NB>;                                 \
    }
// (MPCG_SEL_<g>: the instance's definition if g is this unit's group, nothing otherwise)
#define MPCG_SEL_SOLVE(g, M, S, T, NB, D, W) MPCG_SEL_##g(MPCG_DEF_SOLVE(g, M, S, T, NB, D, W))
#define MPCG_SEL_RESUME(g, M, S, T, NB) MPCG_SEL_##g(MPCG_DEF_RESUME(g, M, S, T, NB))
#define MPCG_SEL_WARM(g, M, S, T, NB, D, W) MPCG_SEL_##g(MPCG_DEF_WARM(g, M, S, T, NB, D, W))
#define MPCG_SEL_PP_SOLVE(g, M, S, T, NB, D, W) MPCG_SEL_##g(MPCG_DEF_PP_SOLVE(g, M, S, T, NB, D, W))
#define MPCG_SEL_PP_RESUME(g, M, S, T, NB) MPCG_SEL_##g(MPCG_DEF_PP_RESUME(g, M, S, T, NB))
#define MPCG_SEL_START(g, M, S, T, NB, D, W) MPCG_SEL_##g(MPCG_DEF_START(g, M, S, T, NB, D, W))
#define MPCG_SEL_START_RESUME(g, M, S, T, NB) MPCG_SEL_##g(MPCG_DEF_START_RESUME(g, M, S, T, NB))
#if MPCG_INST == 0
#define MPCG_SEL_0(x) x
#else
#define MPCG_SEL_0(x)
#endif
#if MPCG_INST == 1
#define MPCG_SEL_1(x) x
#else
#define MPCG_SEL_1(x)
#endif
#if MPCG_INST == 2
#define MPCG_SEL_2(x) x
#else
#define MPCG_SEL_2(x)
#endif
#if MPCG_INST == 3
#define MPCG_SEL_3(x) x
#else
#define MPCG_SEL_3(x)
#endif
#if MPCG_INST == 4
#define MPCG_SEL_4(x) x
#else
#define MPCG_SEL_4(x)
#endif
#if MPCG_INST == 5
#define MPCG_SEL_5(x) x
#else
#define MPCG_SEL_5(x)
#endif
#if MPCG_INST == 6
#define MPCG_SEL_6(x) x
#else
#define MPCG_SEL_6(x)
#endif
#if MPCG_INST == 7
#define MPCG_SEL_7(x) x
#else
#define MPCG_SEL_7(x)
#endif
#if MPCG_INST == 8
#define MPCG_SEL_8(x) x
#else
#define MPCG_SEL_8(x)
#endif
#if MPCG_INST == 9
#define MPCG_SEL_9(x) x
#else
#define MPCG_SEL_9(x)
#endif
#if MPCG_INST == 10
#define MPCG_SEL_10(x) x
#else
#define MPCG_SEL_10(x)
#endif
#if MPCG_INST == 11
#define MPCG_SEL_11(x) x
#else
#define MPCG_SEL_11(x)
#endif
#if MPCG_INST == 12
#define MPCG_SEL_12(x) x
#else
#define MPCG_SEL_12(x)
#endif
#if MPCG_INST == 13
#define MPCG_SEL_13(x) x
#else
#define MPCG_SEL_13(x)
#endif
#if MPCG_INST == 14
#define MPCG_SEL_14(x) x
#else
#define MPCG_SEL_14(x)
#endif
#if MPCG_INST == 15
#define MPCG_SEL_15(x) x
#else
#define MPCG_SEL_15(x)
#endif
#if MPCG_INST == 16
#define MPCG_SEL_16(x) x
#else
#define MPCG_SEL_16(x)
#endif
#if MPCG_INST == 17
#define MPCG_SEL_17(x) x
#else
#define MPCG_SEL_17(x)
#endif
#if MPCG_INST == 18
#define MPCG_SEL_18(x) x
#else
#define MPCG_SEL_18(x)
#endif
#if MPCG_INST == 19
#define MPCG_SEL_19(x) x
#else
#define MPCG_SEL_19(x)
#endif
#if MPCG_INST == 20
#define MPCG_SEL_20(x) x
#else
#define MPCG_SEL_20(x)
#endif
#if MPCG_INST == 21
#define MPCG_SEL_21(x) x
#else
#define MPCG_SEL_21(x)
#endif
#if MPCG_INST == 22
#define MPCG_SEL_22(x) x
#else
#define MPCG_SEL_22(x)
#endif
#if MPCG_INST == 23
#define MPCG_SEL_23(x) x
#else
#define MPCG_SEL_23(x)
#endif
#if MPCG_INST == 24
#define MPCG_SEL_24(x) x
#else
#define MPCG_SEL_24(x)
#endif
#if MPCG_INST == 25
#define MPCG_SEL_25(x) x
#else
#define MPCG_SEL_25(x)
#endif
#if MPCG_INST == 26
#define MPCG_SEL_26(x) x
#else
#define MPCG_SEL_26(x)
#endif
#if MPCG_INST == 27
#define MPCG_SEL_27(x) x
#else
#define MPCG_SEL_27(x)
#endif
#if MPCG_INST == 28
#define MPCG_SEL_28(x) x
#else
#define MPCG_SEL_28(x)
#endif
#if MPCG_INST == 29
#define MPCG_SEL_29(x) x
#else
#define MPCG_SEL_29(x)
#endif
#if MPCG_INST == 30
#define MPCG_SEL_30(x) x
#else
#define MPCG_SEL_30(x)
#endif
#if MPCG_INST == 31
#define MPCG_SEL_31(x) x
#else
#define MPCG_SEL_31(x)
#endif
#if MPCG_INST == 32
#define MPCG_SEL_32(x) x
#else
#define MPCG_SEL_32(x)
#endif
#if MPCG_INST == 33
#define MPCG_SEL_33(x) x
#else
#define MPCG_SEL_33(x)
#endif
MPCG_WIDE_SOLVE_INSTANCES(MPCG_SEL_SOLVE)
MPCG_WIDE_RESUME_INSTANCES(MPCG_SEL_RESUME)
MPCG_WIDE_WARM_INSTANCES(MPCG_SEL_WARM)
MPCG_WIDE_PP_SOLVE_INSTANCES(MPCG_SEL_PP_SOLVE)
MPCG_WIDE_PP_RESUME_INSTANCES(MPCG_SEL_PP_RESUME)
MPCG_WIDE_START_INSTANCES(MPCG_SEL_START)
MPCG_WIDE_START_RESUME_INSTANCES(MPCG_SEL_START_RESUME)

}  // namespace mpcg
