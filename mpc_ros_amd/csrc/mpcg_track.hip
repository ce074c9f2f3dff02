// mpc_ros_amd/csrc/mpcg_track.hip -- the caller side of MPC::Solve on the device.
//
// Tracking::findBestPath (mpc_ros/src/driving_state.cpp:175-271) for B robots, one
// robot per lane:
//   waypoints to the vehicle frame (:196-207), cubic polyfit by Householder QR
//   (:210, polyfit :283-300), cte = polyeval(c, 0) (:211), path heading from the
//   first int(0.3 M) waypoint increments (:214-235), delay-mode state prediction
//   (:242-256);
// and the post-processing of the solve (:262-269): w = w0, throttle = a0,
// speed = min(v_fb + throttle dt, REF_V).
//
// Every control tick is one pipeline (mpcg_api.cpp tick): preprocessing, solve, post-processing.
//   preprocessing   k_find_best_path<16|64> / k_find_best_path_long: M waypoints for every robot;
//                   k_find_best_path_n<16|64>: a count per robot in plan rows of M <= 64.  One
//                   body, find_best_path_pass.
//   post-processing k_post: the clamp to the handle's REF_V or to the robot's own.
// mpcg_track_device is the tick alone.  mpcg_track_device_goal runs k_decelerate before it
// (Tracking::deceleration, :121-141: each robot's REF_V and its parameter row, pp_row_write).
// mpcg_rollout_device runs per tick k_plan_window (the plan window from a shared course, the rule
// of mpcg_window.h) and k_rollout_begin (deceleration, the done mark, the row, the logs) before
// it and k_rollout_end (the unicycle, the command's log) after it.  Every launch goes through
// launch_lanes.
//
// The QR runs on MAXM-row arrays (the M waypoint rows followed by zero rows, which
// change no norm or inner product), unrolled so they stay in registers for M <= 16;
// a second instance with MAXM = 64 covers longer plans, and plans beyond 64 waypoints
// (findBestPath takes any length) run the same QR with the matrix in an HBM workspace
// (k_find_best_path_long).  Same operation order as oracle/preprocess.c.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mpcg_internal.h"
#include "mpcg_pp.h"
#include "mpcg_window.h"

namespace mpcg {

template <int MAXM>
__device__ __forceinline__ void polyfit3(int M, const double* xs, const double* ys, double* c) {
    constexpr int n = 4;
    double A[MAXM][n], b[MAXM];
#pragma unroll
    for (int i = 0; i < MAXM; ++i) {
        const bool in = i < M;
        A[i][0] = in ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < n - 1; ++j) A[i][j + 1] = A[i][j] * (in ? xs[i] : 0.0);
        b[i] = in ? ys[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < n; ++k) {
        double nrm = 0.0;
#pragma unroll
        for (int i = k; i < MAXM; ++i) nrm += A[i][k] * A[i][k];
        nrm = sqrt(nrm);
        const double alpha = (A[k][k] > 0) ? -nrm : nrm;
        double vv[MAXM];
#pragma unroll
        for (int i = k; i < MAXM; ++i) vv[i] = (i == k) ? A[k][k] - alpha : A[i][k];
        double vnorm2 = 0.0;
#pragma unroll
        for (int i = k; i < MAXM; ++i) vnorm2 += vv[i] * vv[i];
        const bool skip = (nrm == 0.0) || (vnorm2 == 0.0);
#pragma unroll
        for (int j = k; j < n; ++j) {
            double s = 0.0;
#pragma unroll
            for (int i = k; i < MAXM; ++i) s += vv[i] * A[i][j];
            s = 2.0 * s / vnorm2;
#pragma unroll
            for (int i = k; i < MAXM; ++i) A[i][j] = skip ? A[i][j] : A[i][j] - s * vv[i];
        }
        double s = 0.0;
#pragma unroll
        for (int i = k; i < MAXM; ++i) s += vv[i] * b[i];
        s = 2.0 * s / vnorm2;
#pragma unroll
        for (int i = k; i < MAXM; ++i) b[i] = skip ? b[i] : b[i] - s * vv[i];
    }
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
        double s = b[k];
#pragma unroll
        for (int j = k + 1; j < n; ++j) s -= A[k][j] * c[j];
        c[k] = s / A[k][k];
    }
}

struct TrackArgs {
    int64_t B;
    int M;
    double dt;
    int delay_mode;
    const double* pose;   // [B][3] x, y, yaw
    const double* vel;    // [B][3] v feedback, previous w, previous throttle
    const double* plan;   // [B][M][2]
    double* state;        // [B][6]
    double* coeffs;       // [B][4]
};

__device__ __forceinline__ void finish_state(const TrackArgs& a, int64_t p, double theta, double v, double w,
                                             double throttle, const double* c);

// findBestPath's preprocessing of robot p on a.M waypoints: the body of k_find_best_path, and one
// pass of k_find_best_path_n
template <int MAXM>
__device__ __forceinline__ void find_best_path_pass(const TrackArgs& a, int64_t p) {
    const int M = a.M;
    const double px = a.pose[p * 3 + 0], py = a.pose[p * 3 + 1], theta = a.pose[p * 3 + 2];
    const double v = a.vel[p * 3 + 0], w = a.vel[p * 3 + 1], throttle = a.vel[p * 3 + 2];
    const double* pl = a.plan + p * (int64_t)M * 2;
    const double ct = cos(theta), st = sin(theta);
    double xv[MAXM], yv[MAXM];
#pragma unroll
    for (int i = 0; i < MAXM; ++i) {
        double dx = 0, dy = 0;
        if (i < M) {
            dx = pl[2 * i] - px;
            dy = pl[2 * i + 1] - py;
        }
        xv[i] = dx * ct + dy * st;
        yv[i] = dy * ct - dx * st;
    }
    double c[4];
    polyfit3<MAXM>(M, xv, yv, c);
    finish_state(a, p, theta, v, w, throttle, c);
}

template <int MAXM>
__global__ void __launch_bounds__(64) k_find_best_path(TrackArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    find_best_path_pass<MAXM>(a, p);
}

// Plans of more than 64 waypoints: polyfit3's Householder QR, same operations in the same
// order, on the M x 4 matrix, the right-hand side and the reflector held in HBM
// (element (i, j) of robot p at ws[(6 i + j) B + p]: a wavefront's lanes touch 64
// consecutive doubles); zero rows past M change nothing, so the loops stop at M.
__global__ void __launch_bounds__(64) k_find_best_path_long(TrackArgs a, double* ws) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    const int M = a.M;
    const int64_t B = a.B;
    double* e = ws + p;
#define E(i, j) e[((int64_t)(i) * 6 + (j)) * B]
    const double px = a.pose[p * 3 + 0], py = a.pose[p * 3 + 1], theta = a.pose[p * 3 + 2];
    const double v = a.vel[p * 3 + 0], w = a.vel[p * 3 + 1], throttle = a.vel[p * 3 + 2];
    const double* pl = a.plan + p * (int64_t)M * 2;
    const double ct = cos(theta), st = sin(theta);
    for (int i = 0; i < M; ++i) {
        const double dx = pl[2 * i] - px, dy = pl[2 * i + 1] - py;
        const double xv = dx * ct + dy * st;
        E(i, 0) = 1.0;
        double q = 1.0;
        for (int j = 0; j < 3; ++j) {
            q = q * xv;
            E(i, j + 1) = q;
        }
        E(i, 4) = dy * ct - dx * st;
    }
    for (int k = 0; k < 4; ++k) {
        double nrm = 0.0;
        for (int i = k; i < M; ++i) nrm += E(i, k) * E(i, k);
        nrm = sqrt(nrm);
        const double akk = E(k, k);
        const double alpha = (akk > 0) ? -nrm : nrm;
        double vnorm2 = 0.0;
        for (int i = k; i < M; ++i) {
            const double vi = (i == k) ? akk - alpha : E(i, k);
            E(i, 5) = vi;
            vnorm2 += vi * vi;
        }
        if (nrm == 0.0 || vnorm2 == 0.0) continue;
        for (int j = k; j < 5; ++j) {  // columns k..3, then the right-hand side
            double s = 0.0;
            for (int i = k; i < M; ++i) s += E(i, 5) * E(i, j);
            s = 2.0 * s / vnorm2;
            for (int i = k; i < M; ++i) E(i, j) = E(i, j) - s * E(i, 5);
        }
    }
    double c[4];
    for (int k = 3; k >= 0; --k) {
        double s = E(k, 4);
        for (int j = k + 1; j < 4; ++j) s -= E(k, j) * c[j];
        c[k] = s / E(k, k);
    }
#undef E
    finish_state(a, p, theta, v, w, throttle, c);
}

// cte, the path heading and the (delayed) state from the fitted polynomial
// (driving_state.cpp:211-256)
__device__ __forceinline__ void finish_state(const TrackArgs& a, int64_t p, double theta, double v, double w,
                                             double throttle, const double* c) {
    const int M = a.M;
    const double dt = a.dt;
    const double* pl = a.plan + p * (int64_t)M * 2;
    // polyeval(coeffs, 0.0) with pow(0, k) (driving_state.cpp:302-309): pow(0, 0) = 1
    const double cte = c[0];
    double gx = 0.0, gy = 0.0;
    const int nsample = (int)(M * 0.3);
    for (int i = 1; i < nsample; ++i) {
        gx += pl[2 * i] - pl[2 * (i - 1)];
        gy += pl[2 * i + 1] - pl[2 * (i - 1) + 1];
    }
    double temp_theta = theta;
    const double traj_deg = atan2(gy, gx);
    const double PI = M_PI;
    if (temp_theta <= -PI + traj_deg) temp_theta = temp_theta + 2 * PI;
    double etheta;
    if (gx != 0.0 && gy != 0.0 && temp_theta - traj_deg < 1.8 * PI)
        etheta = temp_theta - traj_deg;
    else
        etheta = 0;
    double* s = a.state + p * 6;
    if (a.delay_mode) {
        const double theta_act = w * dt;
        s[0] = v * dt;
        s[1] = 0;
        s[2] = theta_act;
        s[3] = v + throttle * dt;
        s[4] = cte + v * sin(etheta) * dt;
        s[5] = etheta - theta_act;
    } else {
        s[0] = 0;
        s[1] = 0;
        s[2] = 0;
        s[3] = v;
        s[4] = cte;
        s[5] = etheta;
    }
    double* co = a.coeffs + p * 4;
    co[0] = c[0];
    co[1] = c[1];
    co[2] = c[2];
    co[3] = c[3];
}

// driving_state.cpp:262-269 -> cmd[B][3] = (speed, w, throttle).  The clamp is REF_V: ref_v, or
// the robot's own ref_vs[p] where ref_vs is given (:267-268 reads the map's current entry)
__global__ void __launch_bounds__(64) k_post(int64_t B, double dt, double ref_v, const double* ref_vs,
                                            const double* vel, const double* u0, double* cmd) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= B) return;
    if (ref_vs) ref_v = ref_vs[p];
    const double w = u0[p * 2 + 0], thr = u0[p * 2 + 1];
    double speed = vel[p * 3 + 0] + thr * dt;
    if (speed >= ref_v) speed = ref_v;
    cmd[p * 3 + 0] = speed;
    cmd[p * 3 + 1] = w;
    cmd[p * 3 + 2] = thr;
}

// hypot(x, y) correctly rounded (but for values within ~2^-100 of a rounding boundary): x^2 + y^2
// as an unevaluated sum of two doubles, its square root, and one Newton correction from the
// exact residual.  A host's libm hypot differs between builds by an ulp (with and without FMA);
// the deceleration rule hands this distance on as REF_V, so it is pinned to the exact value.
// Outside the range where the squares neither overflow nor lose bits: the library's hypot.
__device__ __forceinline__ double hypot_cr(double x, double y) {
#pragma clang fp contract(off)
    double a = fabs(x), b = fabs(y);
    if (a < b) {
        const double t = a;
        a = b;
        b = t;
    }
    if (!(a < 1e150) || (b != 0.0 && b < 1e-130)) return hypot(x, y);
    if (a == 0.0) return 0.0;
    const double ah = a * a, al = __builtin_fma(a, a, -ah);
    const double bh = b * b, bl = __builtin_fma(b, b, -bh);
    const double sh = ah + bh, e = bh - (sh - ah);  // (ah >= bh: the sum's rounding error, exactly)
    const double sl = e + (al + bl);
    const double h = sqrt(sh);
    const double r = __builtin_fma(-h, h, sh) + sl;  // (sh - h^2 is exact for a correctly rounded root)
    return h + r / (2.0 * h);
}

// Tracking::deceleration (driving_state.cpp:121-141) for B robots, one per lane: ref_v[b] (in/out,
// the robot's REF_V map entry) from its distance to its goal and its feedback speed, then the
// robot's parameter row: the handle's row with REF_V = ref_v[b] (pp_row_write).
__global__ void __launch_bounds__(64) k_decelerate(int64_t B, const double* pose, const double* vel, const double* goal,
                                                  double* ref_v, double max_throttle, double max_speed,
                                                  double min_speed, PPRow row, double* rows) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= B) return;
    const double dist = hypot_cr(pose[p * 3 + 0] - goal[p * 2 + 0], pose[p * 3 + 1] - goal[p * 2 + 1]);
    const double rv = decelerate(dist, vel[p * 3 + 0], max_throttle, max_speed, min_speed, ref_v[p]);
    ref_v[p] = rv;
    pp_row_write(row, rv, true, rows + p * MPCG_PP_FIELDS);
}

// ---- The closed loop on the device (mpcg_rollout_device): the plan window from a shared course,
// the preprocessing with a waypoint count per robot, and the two ends of a rollout tick. ----

// MPCPlannerROS::getCutOffPlan and downSamplePlan (mpcg_window.h) for B robots, one per lane, each
// on one of C shared courses: cursor [B] (in/out), plan [B][Mmax][2] (rows past the count are 0),
// count [B], start [B] (may be null).  A robot whose course index, course length or cursor is out
// of range reads no course: count 0, cursor unchanged.
struct WindowArgs {
    int64_t B;
    const double* courses;      // [C][Gmax][2]
    const int32_t* course_len;  // [C]
    const int32_t* course_of;   // [B]
    int C, Gmax;
    const double* pose;         // [B][3]
    int window_wp, stride, Mmax;
    int32_t* cursor;
    double* plan;
    int32_t* count;
    int32_t* start;
};

// robot p's course, or null where it has none (its index or the course's length out of range)
__device__ __forceinline__ const double* course_of_robot(const double* courses, const int32_t* course_len,
                                                         const int32_t* course_of, int C, int Gmax, int64_t p, int* G) {
    const int co = course_of[p];
    if (co < 0 || co >= C) return nullptr;
    *G = course_len[co];
    if (*G < 1 || *G > Gmax) return nullptr;
    return courses + (int64_t)co * Gmax * 2;
}

__global__ void __launch_bounds__(64) k_plan_window(WindowArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    int G = 0;
    const double* course = course_of_robot(a.courses, a.course_len, a.course_of, a.C, a.Gmax, p, &G);
    const int c = a.cursor[p];
    PlanWindow w{c, 0, 0, 0};
    if (course && c >= 0 && c < G)
        w = plan_window(course, G, c, a.pose[p * 3 + 0], a.pose[p * 3 + 1], a.window_wp, a.stride);
    plan_window_copy(course, w, a.stride, a.Mmax, a.plan + p * (int64_t)a.Mmax * 2);
    a.cursor[p] = w.cursor;
    a.count[p] = w.count;
    if (a.start) a.start[p] = w.start;
}

// k_find_best_path with robot p's own waypoint count: a.M is the plan's row stride Mmax
// (<= MAXM), count[p] the rows that hold waypoints.  The heading from the first int(0.3 count)
// increments and everything after it use the robot's count.  A robot with fewer than 4 waypoints
// (polyfit asserts order 3 <= M - 1, driving_state.cpp:286), or a count beyond the stride, is not
// fitted: its state and coeffs are 0.
// The wavefront makes one pass per distinct count among its robots, the count wave-uniform in
// each (the first waiting lane's; the lanes that hold it run the pass): the pass is
// k_find_best_path's body (find_best_path_pass) on a scalar M, so a robot's result does not
// depend on its neighbours' counts, and a batch of one count is that kernel's arithmetic.  Most
// robots of a fleet hold a full window, so a wavefront makes one to three passes.
template <int MAXM>
__global__ void __launch_bounds__(64) k_find_best_path_n(TrackArgs a, const int32_t* count) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    const int Mp = count[p];
    if (Mp < 4 || Mp > a.M) {
        for (int j = 0; j < 6; ++j) a.state[p * 6 + j] = 0.0;
        for (int j = 0; j < 4; ++j) a.coeffs[p * 4 + j] = 0.0;
        return;
    }
    // (the loop is wave-uniform: todo holds the lanes that still wait, and its lowest lane always
    // matches its own count, so every pass retires at least that lane)
    unsigned long long todo = __ballot(1);
    while (todo) {
        const int M = __builtin_amdgcn_readlane(Mp, __ffsll(todo) - 1);
        // (the lanes that hold M, as a mask: under a test `Mp == M` the compiler would put the
        // lane's own Mp in M's place, and the pass would run on a per-lane count again)
        const unsigned long long same = __ballot(Mp == M);
        todo &= ~same;
        if ((same >> threadIdx.x) & 1) {
            // (the pass reads robot p's plan at plan + 2 p M: rows of M, here of a.M)
            TrackArgs r = a;
            r.M = M;
            r.plan = a.plan + p * (int64_t)(a.M - M) * 2;
            find_best_path_pass<MAXM>(r, p);
        }
    }
}

// One rollout tick around the solve.  k_rollout_begin, after the window: Tracking::deceleration
// towards the goal (the course's last waypoint), the done mark, the robot's parameter row and the
// tick's inputs into the logs.  k_rollout_end, after the post-processing: the command of a done
// robot is 0; the unicycle over one control period; the command into the log.
// (RolloutArgs: mpcg_internal.h)

__global__ void __launch_bounds__(64) k_rollout_begin(RolloutArgs a, PPRow row) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    int G = 0;
    const double* course = course_of_robot(a.courses, a.course_len, a.course_of, a.C, a.Gmax, p, &G);
    const double x = a.pose[p * 3 + 0], y = a.pose[p * 3 + 1], v = a.vel[p * 3 + 0];
    double rv = a.ref_v[p];
    bool at_goal = false;
    if (course) {
        const double dist = hypot_cr(x - course[2 * (G - 1)], y - course[2 * (G - 1) + 1]);
        rv = decelerate(dist, v, a.max_throttle, a.max_speed, a.min_speed, rv);
        a.ref_v[p] = rv;
        at_goal = dist <= a.goal_tol;
    }
    const int n = a.count[p];
    int dn = a.done[p];
    if (dn == 0 && (n < 4 || at_goal)) {
        dn = a.tick + 1;
        a.done[p] = dn;
    }
    // (a done robot's row is invalid: its problem ends at iteration 0 with zero controls)
    pp_row_write(row, rv, dn == 0, a.rows + p * MPCG_PP_FIELDS);
    if (a.log_pose)
        for (int j = 0; j < 3; ++j) a.log_pose[p * 3 + j] = a.pose[p * 3 + j];
    if (a.log_vel)
        for (int j = 0; j < 3; ++j) a.log_vel[p * 3 + j] = a.vel[p * 3 + j];
    if (a.log_ref_v) a.log_ref_v[p] = rv;
    if (a.log_cursor) a.log_cursor[p] = a.cursor[p];
    if (a.log_start) a.log_start[p] = a.start[p];
    if (a.log_count) a.log_count[p] = n;
}

__global__ void __launch_bounds__(64) k_rollout_end(RolloutArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= a.B) return;
    const bool dn = a.done[p] != 0;
    const double speed = dn ? 0.0 : a.cmd[p * 3 + 0];
    const double w = dn ? 0.0 : a.cmd[p * 3 + 1];
    const double thr = dn ? 0.0 : a.cmd[p * 3 + 2];
    if (a.log_cmd) {
        a.log_cmd[p * 3 + 0] = speed;
        a.log_cmd[p * 3 + 1] = w;
        a.log_cmd[p * 3 + 2] = thr;
    }
    if (!a.integrate) return;
    if (!dn) {  // (a done robot's pose is frozen)
        const double yaw = a.pose[p * 3 + 2];
        a.pose[p * 3 + 0] += speed * cos(yaw) * a.dt;
        a.pose[p * 3 + 1] += speed * sin(yaw) * a.dt;
        const double next = yaw + w * a.dt;
        a.pose[p * 3 + 2] = atan2(sin(next), cos(next));
    }
    a.vel[p * 3 + 0] = speed;
    a.vel[p * 3 + 1] = w;
    a.vel[p * 3 + 2] = thr;
}

// the launch of every kernel here: one robot per lane, 64 per workgroup; nothing for no robots
template <class Kernel, class... Args>
static hipError_t launch_lanes(Kernel kernel, int64_t B, hipStream_t stream, const Args&... args) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, args...);
    return hipGetLastError();
}

hipError_t launch_plan_window(int64_t B, const double* courses, const int32_t* course_len, const int32_t* course_of,
                              int C, int Gmax, const double* pose, int window_wp, int stride, int Mmax,
                              int32_t* cursor, double* plan, int32_t* count, int32_t* start, hipStream_t stream) {
    const WindowArgs a{B, courses, course_len, course_of, C, Gmax, pose, window_wp, stride, Mmax, cursor, plan, count,
                       start};
    return launch_lanes(k_plan_window, B, stream, a);
}

size_t find_best_path_ws_bytes(int64_t B, int M) { return M > 64 ? sizeof(double) * 6 * (size_t)M * (size_t)B : 0; }

hipError_t launch_find_best_path(int64_t B, int M, const int32_t* count, double dt, int delay_mode, const double* pose,
                                 const double* vel, const double* plan, double* state, double* coeffs, double* ws,
                                 hipStream_t stream) {
    const TrackArgs a{B, M, dt, delay_mode, pose, vel, plan, state, coeffs};
    if (count) {
        if (M > kWindowMaxM) return hipErrorInvalidValue;
        return M <= 16 ? launch_lanes(k_find_best_path_n<16>, B, stream, a, count)
                       : launch_lanes(k_find_best_path_n<64>, B, stream, a, count);
    }
    if (M <= 16) return launch_lanes(k_find_best_path<16>, B, stream, a);
    if (M <= 64) return launch_lanes(k_find_best_path<64>, B, stream, a);
    if (!ws) return hipErrorInvalidValue;
    return launch_lanes(k_find_best_path_long, B, stream, a, ws);
}

hipError_t launch_post(int64_t B, double dt, double ref_v, const double* ref_vs, const double* vel, const double* u0,
                       double* cmd, hipStream_t stream) {
    return launch_lanes(k_post, B, stream, B, dt, ref_v, ref_vs, vel, u0, cmd);
}

hipError_t launch_decelerate(int64_t B, const double* pose, const double* vel, const double* goal, double* ref_v,
                             double max_throttle, double max_speed, double min_speed, const PPRow& row, double* rows,
                             hipStream_t stream) {
    return launch_lanes(k_decelerate, B, stream, B, pose, vel, goal, ref_v, max_throttle, max_speed, min_speed, row,
                        rows);
}

hipError_t launch_rollout_begin(const RolloutArgs& a, const PPRow& row, hipStream_t stream) {
    return launch_lanes(k_rollout_begin, a.B, stream, a, row);
}

hipError_t launch_rollout_end(const RolloutArgs& a, hipStream_t stream) {
    return launch_lanes(k_rollout_end, a.B, stream, a);
}

}  // namespace mpcg
