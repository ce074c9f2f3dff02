// mpc_ros_amd/csrc/mpcg_wide_inst.hip -- the solver kernel instances, one group per
// translation unit: build.py compiles this file once per MPCG_INST value (0 .. kWideGroups - 1,
// in parallel) and links the objects into libmpcg.so.  The instances and their groups are the
// rows of wide_plan.h's MPCG_WIDE_INSTANCES.
#include "mpcg_wide_kern.h"

#ifndef MPCG_INST
#error "compile with -DMPCG_INST=<group>"
#endif

namespace mpcg {

// the kernel of a row
template <int K, int M, bool S, class T, int NB, bool D, int W>
static const void* row_kernel() {
    if constexpr (K == SOLVE) return (const void*)k_solve_wide<M, S, T, NB, D, W>;
    else if constexpr (K == WARM) return (const void*)k_warm_wide<M, S, T, NB, D, W>;
    else if constexpr (K == PP_SOLVE) return (const void*)k_solve_wide_pp<M, S, T, NB, D, W>;
    else if constexpr (K == START) return (const void*)k_start_wide<M, S, T, NB, D, W>;
    else if constexpr (K == PP_RESUME) return (const void*)k_resume_wide<K, M, S, T, NB, const double*>;
    else if constexpr (K == START_RESUME) return (const void*)k_resume_wide<K, M, S, T, NB, StartIn>;
    else return (const void*)k_resume_wide<RESUME, M, S, T, NB>;
}
// Every row of the list counts; a row of group G stores its kernel.  The condition depends on
// G, so a unit instantiates -- compiles -- the kernels of its own group only.
#define MPCG_ROW_FILL(g, K, M, S, T, NB, D, W)                              \
    {                                                                       \
        constexpr int g_ = g;                                               \
        if constexpr (g_ == G) t[i] = row_kernel<K, M, S, T, NB, D, W>();   \
        ++i;                                                                \
    }
template <int G>
void wide_group(const void** t) {
    int i = 0;
    MPCG_WIDE_INSTANCES(MPCG_ROW_FILL)
}
template void wide_group<MPCG_INST>(const void**);

}  // namespace mpcg
