// mpc_ros_amd/csrc/mpcg_window.h -- the plan window of one robot on its course: the cut of
// MPCPlannerROS::getCutOffPlan (mpc_ros/src/mpc_planner_ros.cpp:266-291) and the down-sampling of
// downSamplePlan (:365-391), on a plan addressed by index instead of erased.  Host and device:
// mpcg_api.cpp (mpcg_plan_window) and the kernel (k_plan_window) run the same code.
#ifndef MPCG_WINDOW_H
#define MPCG_WINDOW_H

#include "ipm_core.h"

namespace mpcg {

// most sampled waypoints of a window the device takes (the ragged preprocessing's largest instance)
constexpr int kWindowMaxM = 64;

struct PlanWindow {
    int cursor;  // the robot's place on the course after the cut: max(c, start - 1)
    int start;   // the first waypoint kept
    int W;       // course waypoints in the window: min(window_wp, G - start)
    int count;   // sampled waypoints: ceil(W / stride) + 1, or 0 for an empty window
};

// Mmax = ceil(window_wp / stride) + 1, the rows of a robot's sampled plan (window_wp, stride >= 1)
MPCG_HD int64_t plan_window_mmax(int window_wp, int stride) {
    return ((int64_t)window_wp + stride - 1) / stride + 1;
}

// The cut from cursor c (0 <= c < G) at the pose (x, y): the reference erases waypoints from the
// front while their squared distance does not increase (:276-287, max_distance_sq starts at the
// literal 10e5), the nearest one included, so the window starts at the first waypoint whose
// distance increases.  The walk ends at G.  (No contraction: the distances are the reference's
// two products and one sum, the same on the host and on the device.)
MPCG_HD PlanWindow plan_window(const double* course, int G, int c, double x, double y, int window_wp, int stride) {
#pragma clang fp contract(off)
    double d_prev = 10e5;
    int i = c;
    while (i < G) {
        const double x_diff = x - course[2 * i], y_diff = y - course[2 * i + 1];
        const double d = x_diff * x_diff + y_diff * y_diff;
        if (d_prev < d) break;
        d_prev = d;
        ++i;
    }
    PlanWindow w;
    w.start = i;
    w.cursor = i - 1 > c ? i - 1 : c;
    w.W = G - i < window_wp ? G - i : window_wp;
    w.count = w.W > 0 ? (int)plan_window_mmax(w.W, stride) : 0;
    return w;
}

// The course index of sampled waypoint j < count: every stride-th waypoint of the window, then
// its last one once more (downSamplePlan pushes cutoff_plan.back() unconditionally, :390, so the
// last waypoint appears twice where W - 1 is a multiple of the stride).
MPCG_HD int plan_window_index(const PlanWindow& w, int stride, int j) {
    return j < w.count - 1 ? w.start + j * stride : w.start + w.W - 1;
}

// Rows [Mmax][2] of the sampled plan: the count waypoints, then zeros.
MPCG_HD void plan_window_copy(const double* course, const PlanWindow& w, int stride, int Mmax, double* plan) {
    for (int j = 0; j < Mmax; ++j) {
        const bool in = j < w.count;
        const int g = in ? plan_window_index(w, stride, j) : 0;
        plan[2 * j] = in ? course[2 * g] : 0.0;
        plan[2 * j + 1] = in ? course[2 * g + 1] : 0.0;
    }
}

}  // namespace mpcg
#endif
