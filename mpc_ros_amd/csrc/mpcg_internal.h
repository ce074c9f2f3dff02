// mpc_ros_amd/csrc/mpcg_internal.h -- declarations shared by the kernels and the C-ABI layer.
#ifndef MPCG_INTERNAL_H
#define MPCG_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "wide_plan.h"

namespace mpcg {

// mpcg_last_error()'s message for this thread; returns code
int set_error(int code, const std::string& msg);

// One problem per wavefront (mpcg_wide.hip; the plan -- instance choice, workspace layout,
// wide_lds_bytes, kOrderMinBatch -- is wide_plan.h).
// HBM workspace of a batch of B (watchdog, acceptable point, second-order corrections,
// soft restoration, the restoration phase: rare paths that must not cost LDS): one slot
// per wavefront the device holds resident, claimed by each problem's wavefront
// (SolveLayout::total for the current device)
size_t wide_spill_bytes(const IpmParams& P, int64_t B);
// The streams and events a solve forks work onto (each joined back into the caller's stream
// before the launch returns): aux -- the resume workers of the restoration phase, and the fp32
// configuration's head (the problems the solve order ranks longest, solved in fp64 while the
// fp32 phase runs); aux2 -- the head's own resume workers.
struct WideStreams {
    hipStream_t aux = nullptr, aux2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
};
// A started solve (mpcg_solve_device_start): the start records [B][solution_elems(N)], the mode
// of each problem, the barrier parameter of each FULL start (or null: mu_init) and the mode that
// ran (or null), all on the device -- the k_start_wide / k_resume_wide<START_RESUME> instances;
// fp64 only
struct WideStart {
    const double* rec = nullptr;
    const int32_t* mode = nullptr;
    const double* mu0 = nullptr;
    int32_t* used = nullptr;
};
// What one solve of B problems reads and writes, all on the device.  Required: state [B][6],
// coeffs [B][4], u0 [B][2]; every other pointer may be null.
struct SolveRequest {
    int64_t B = 0;
    const double *state = nullptr, *coeffs = nullptr;
    // a parameter row per problem, [B][16] doubles in include/mpcg.h's MPCG_PP_* order -- the
    // k_solve_wide_pp / k_resume_wide<PP_RESUME> instances; fp64 only
    const double* rows = nullptr;
    double *u0 = nullptr, *traj = nullptr;  // traj [B][3][N]
    int32_t* status = nullptr;
    double* obj = nullptr;
    int32_t *iters = nullptr, *diag = nullptr;  // diag [B][4]
    // the solution records [B][solution_elems(N)], written by every ending's write_out --
    // WideSolver::solution_out (may be start.rec: a record is read before its problem's solve)
    double* sol = nullptr;
    WideStart start;  // (rec and mode given: a started solve)
    bool started() const { return start.rec || start.mode; }
};
hipError_t launch_wide_solve(const IpmParams& P, const SolveRequest& rq, const int32_t* order, void* spill,
                             size_t spill_bytes, hipStream_t stream, const WideStreams& ws = WideStreams(),
                             const char** kernel_name = nullptr);
// The certificate (mpcg_kkt.hip): cert [B][4] from the NLP alone at the records sol; `row` the
// handle's per-problem fields, rows [B][16] (or null) a row per problem.
struct PPRow;
hipError_t launch_kkt_certify(int64_t B, int N, int model, const PPRow& row, const double* rows, const double* state,
                              const double* coeffs, const double* sol, double* cert, hipStream_t stream);
// The feedback gains (mpcg_sens.hip): gain [B][2][10], dx [B][10][8N-2] (or null) and info [B] (or
// null) at the records sol; cvt, brf: the handle's constr_viol_tol and bound_relax_factor.  And the
// correction u = clip(u0 + gain [dstate; dcoeffs]) (dcoeffs or null), one robot per lane.
hipError_t launch_sens(int64_t B, int N, int model, const PPRow& row, double cvt, double brf, const double* rows,
                       const double* coeffs, const double* sol, double* gain, double* dx, int32_t* info,
                       hipStream_t stream);
hipError_t launch_sens_apply(int64_t B, const PPRow& row, const double* rows, const double* gain, const double* u0,
                             const double* dstate, const double* dcoeffs, double* u, hipStream_t stream);
// The shift rule (mpcg_shift.hip, mpcg_shift.h): B records in -> out (may alias) towards the
// problems (state, coeffs, row / rows) by motion [B][3]; mask [B] (or null) 0: the record copied.
hipError_t launch_shift_solution(int64_t B, int N, int model, const PPRow& row, const double* rows, const double* state,
                                 const double* coeffs, const double* motion, const int32_t* mask, const double* in,
                                 double* out, hipStream_t stream);
// The warm rollout's two kernels around the solve.  Before it: robot b's carried record shifted in
// place by the motion from carry_pose[b] to pose[b] where carry_ok[b] != 0, done[b] == 0 and
// start_mode != COLD (modes[b] = start_mode, else COLD), mu0s[b] = mu0, carry_pose[b] = pose[b]
// for a running robot.  After it: carry_ok[b] = (done[b] == 0 and status[b] is 1 or 4).
hipError_t launch_shift_rollout(int64_t B, int N, int model, int start_mode, double mu0, const double* rows,
                                const double* state, const double* coeffs, const double* pose, const int32_t* done,
                                const int32_t* carry_ok, double* carry_pose, double* carry_sol, int32_t* modes,
                                double* mu0s, hipStream_t stream);
hipError_t launch_carry_flag(int64_t B, const int32_t* done, const int32_t* status, int32_t* carry_ok,
                             hipStream_t stream);
// Solve order (expected-longest first): device buffer bytes for B problems, and the
// launch that writes the workgroup -> problem map into `buf` (returned in *order).
size_t wide_sched_bytes(int64_t B);
hipError_t launch_wide_order(int64_t B, const double* coeffs, void* buf, size_t bytes, int32_t** order,
                             hipStream_t stream);

// A control tick's lane kernels (mpcg_track.hip; the pipeline is mpcg_api.cpp tick).
// findBestPath's preprocessing: count null -- M waypoints for every robot (M > 64: ws holds
// find_best_path_ws_bytes(B, M) bytes of device scratch); else count[p] waypoints for robot p in
// plan rows of M (<= 64).
size_t find_best_path_ws_bytes(int64_t B, int M);
hipError_t launch_find_best_path(int64_t B, int M, const int32_t* count, double dt, int delay_mode, const double* pose,
                                 const double* vel, const double* plan, double* state, double* coeffs, double* ws,
                                 hipStream_t stream);
// the post-processing: the speed clamp is ref_v, or the robot's own ref_vs[b] where ref_vs is given
hipError_t launch_post(int64_t B, double dt, double ref_v, const double* ref_vs, const double* vel, const double* u0,
                       double* cmd, hipStream_t stream);
// The tick with a goal per robot (mpcg_track_device_goal): Tracking::deceleration on ref_v [B]
// (in/out) and each robot's parameter row -- `row` with REF_V = ref_v[b] -- into rows [B][16].
struct PPRow;
hipError_t launch_decelerate(int64_t B, const double* pose, const double* vel, const double* goal, double* ref_v,
                             double max_throttle, double max_speed, double min_speed, const PPRow& row, double* rows,
                             hipStream_t stream);

// The closed loop on the device (mpcg_track.hip; the window rule is mpcg_window.h).
// The plan window of B robots on C shared courses [C][Gmax][2]: cursor [B] in/out, plan
// [B][Mmax][2] (rows past the count are 0), count [B], start [B] (may be null).
hipError_t launch_plan_window(int64_t B, const double* courses, const int32_t* course_len, const int32_t* course_of,
                              int C, int Gmax, const double* pose, int window_wp, int stride, int Mmax,
                              int32_t* cursor, double* plan, int32_t* count, int32_t* start, hipStream_t stream);
// One rollout tick around the solve.  begin, after the window: Tracking::deceleration towards
// the goal (the course's last waypoint), the done mark, the robot's parameter row (`row` with
// REF_V = ref_v[b]; a done robot's is invalid) and the tick's inputs into the logs.  end, after
// the post-processing: a done robot's command is 0; the unicycle over one control period; the
// command into the log.
struct RolloutArgs {
    int64_t B;
    int tick;  // index within this call
    const double* courses;
    const int32_t* course_len;
    const int32_t* course_of;
    int C, Gmax;
    double goal_tol, max_throttle, max_speed, min_speed, dt;
    int integrate;
    double* pose;           // [B][3] in/out
    double* vel;            // [B][3] in/out
    const int32_t* cursor;  // [B] (after the cut)
    const int32_t* start;   // [B]
    const int32_t* count;   // [B]
    double* ref_v;          // [B] in/out
    int32_t* done;          // [B] in/out
    double* rows;           // [B][16]
    const double* cmd;      // [B][3] (the post-processing's)
    // this tick's rows of the logs, each may be null
    double *log_pose, *log_vel, *log_cmd, *log_ref_v;
    int32_t *log_cursor, *log_start, *log_count;
};
hipError_t launch_rollout_begin(const RolloutArgs& a, const PPRow& row, hipStream_t stream);
hipError_t launch_rollout_end(const RolloutArgs& a, hipStream_t stream);

// The benchmark's synthetic robots (mpcg_synth.hip): the lemniscate's arc-length table (host,
// once) and the per-robot pose / velocities / plan from (seed, global index)
void synth_arc_table(std::vector<double>& t, std::vector<double>& s);
int synth_arc_len();
hipError_t launch_synth_infinity(uint64_t seed, int64_t start, int64_t B, int M, const double* arc_t,
                                 const double* arc_s, double* pose, double* vel, double* plan, hipStream_t stream);

}  // namespace mpcg
#endif
