/*
 * include/mpcg.h -- C-ABI of the MI355X batched NMPC solver (libmpcg.so).
 *
 * Drop-in boundary for the hot path of OkDoky/mpc_ros: the call
 *     vector<double> MPC::Solve(Eigen::VectorXd state, Eigen::VectorXd coeffs)
 * (mpc_ros/include/mpc_planner.h:31, mpc_ros/src/mpc_planner.cpp:265-402), which
 * tapes FG_eval with CppAD and solves the NLP with Ipopt 3.12.8 through
 * CppAD::ipopt::solve (mpc_ros/include/cppad/ipopt/solve.hpp:419-589).  Here a
 * batch of B independent problems is solved on one GPU by hand-written CDNA4 HIP
 * kernels running the same interior-point algorithm (mpc_ros_amd/csrc/ipm_core.h).
 *
 * Plain C types only; every pointer is caller-owned.  Return codes: 0 = ok,
 * negative = API / HIP error (message in mpcg_last_error()).  Per-problem solver
 * outcomes are reported in `status` with CppAD::ipopt::solve_result::status_type
 * numbering (mpc_ros/include/cppad/ipopt/solve_result.hpp:30-46): 1 success,
 * 2 maxiter_exceeded, 3 stop_at_tiny_step, 4 stop_at_acceptable_point,
 * 5 local_infeasibility and 7 feasible_point_found (the feasibility-restoration phase
 * converged without returning to the problem), 9 restoration_failure (the restoration
 * phase's line search failed), 10 error_in_step_computation, 11 invalid_number_detected,
 * 14 unknown (Ipopt's CPUTIME_EXCEEDED, solve_callback.hpp:1165-1167: the max_cpu_time
 * budget below).  As in the reference (mpc_planner.cpp:378, the status is computed and
 * then ignored), the last iterate is always returned.
 *
 * Device-side checks: every index a kernel reads from device memory (the solve order, the
 * workspace's slot and park-area counters and lists, a parked entry's problem tag) is
 * range-checked before use.  A value out of range -- a workspace corrupted or reused by
 * concurrent work outside stream order -- stops the kernel with a trap (the resume and
 * bookkeeping kernels print the value and its bound first); the stream then reports a HIP
 * error (a later call returns -2) and, as after any device fault, the process's HIP context
 * is unusable.
 *
 * Threading: one handle per thread; mpcg_set_params must not run concurrently with
 * a solve on the same handle (the reference has an unsynchronised writer here,
 * SURVEY.md §3.3 -- this API makes the ordering the caller's explicit job).  A handle's
 * device scratch (solve order, spill areas, staging) is used stream-ordered: a solve on a
 * different stream than the handle's previous one first waits for that previous work
 * (an event), so one thread may queue solves on several streams.
 *
 * Integration (cgo/ctypes/C++ stubs): INTEGRATION.md.
 */
#ifndef MPCG_H
#define MPCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCG_ABI_VERSION 2

/* The 15 keys of the reference's parameter map (DrivingStateContext::updateMpcConfigs,
 * mpc_ros/src/driving_state.cpp:65-79; MPC::LoadParams mpc_planner.cpp:243-262;
 * FG_eval::LoadParams mpc_planner.cpp:71-97), plus the Ipopt options the reference
 * leaves at their defaults (mpc_planner.cpp:356-368). */
typedef struct mpcg_params {
    int32_t steps;            /* "STEPS": horizon N (double truncated to int, :74, :247) */
    int32_t model;            /* 0 = differential drive (FG_eval); 1 = kinematic bicycle: the control
                                 w is the steering angle (|w| <= ANGVEL) and the heading rows turn
                                 by v w / wheelbase dt (strategy WAVE only) */
    double dt;                /* "DT" */
    double ref_cte;           /* "REF_CTE" */
    double ref_etheta;        /* "REF_ETHETA" */
    double ref_v;             /* "REF_V" */
    double w_cte;             /* "W_CTE" */
    double w_etheta;          /* "W_EPSI" */
    double w_v;               /* "W_V" */
    double w_angvel;          /* "W_ANGVEL" */
    double w_accel;           /* "W_A" */
    double w_angvel_d;        /* "W_DANGVEL" */
    double w_accel_d;         /* "W_DA" */
    double max_angvel;        /* "ANGVEL" */
    double max_throttle;      /* "MAXTHR" */
    double bound;             /* "BOUND" */
    /* Ipopt 3.12 defaults unless changed */
    double tol;               /* 1e-8 */
    int32_t max_iter;         /* 3000 */
    int32_t filter_cap;       /* filter entries held in LDS per problem (64); 448 more are kept in
                                 the HBM workspace, so the oldest entry is dropped only beyond
                                 filter_cap + 448 non-dominated entries (counted in diag[:, 1];
                                 Ipopt's filter is unbounded).  Results are independent of
                                 filter_cap while fewer than filter_cap + 448 entries are held */
    double bound_relax_factor;/* 1e-8 */
    double mu_init;           /* 0.1 */
    double wheelbase;         /* model 1 only: Lf [m] */
    /* "max_cpu_time" (the reference sets 0.5 s, mpc_planner.cpp:368): applied as the number of
     * iterations the reference's Solve affords in that time at this horizon, so that results
     * are deterministic: (max_cpu_time - CppAD taping) / (CppAD derivative evaluations + Ipopt's
     * own iteration work) -- taping and derivatives measured in the survey (1.52 ms and
     * 0.225 ms per iteration at N = 20), Ipopt's KKT factorisation, solve and line search
     * calibrated at 5.14 us per stage (0.103 ms at N = 20): 1,520 iterations at N = 20, 737 at
     * N = 40.  Beyond it the status is 14 (unknown) with the last iterate.  >= 1e6: no budget
     * (Ipopt's "no limit"). */
    double max_cpu_time;
    /* Ipopt 3.12 defaults (the reference leaves them untouched) */
    double acceptable_tol;             /* 1e-6 */
    double acceptable_dual_inf_tol;    /* 1e10 */
    double acceptable_constr_viol_tol; /* 1e-2 */
    double acceptable_compl_inf_tol;   /* 1e-2 */
    double acceptable_obj_change_tol;  /* 1e20 */
    double kappa_soc;                  /* 0.99 */
    double soft_resto_pderror_reduction_factor; /* 0.9999 (0: no soft restoration) */
    double obj_max_inc;                /* 5 */
    double tiny_step_tol;              /* 10 eps */
    double tiny_step_y_tol;            /* 1e-2 */
    double dual_inf_tol;               /* 1 (unscaled dual infeasibility at termination) */
    double constr_viol_tol;            /* 1e-4 (unscaled constraint violation; caps the bound relaxation) */
    double compl_inf_tol;              /* 1e-4 (unscaled complementarity; mu_min = min(tol, this x objective scaling) / 11;
                                          precision 1: min(tol, this) / 11) */
    int32_t acceptable_iter;           /* 15 (0: no acceptable termination) */
    int32_t max_soc;                   /* 4 (0: no second-order corrections) */
    int32_t watchdog_shortened_iter_trigger; /* 10 (0: no watchdog) */
    int32_t watchdog_trial_iter_max;   /* 3 */
    int32_t max_soft_resto_iters;      /* 10 */
    int32_t max_filter_resets;         /* 5 */
    int32_t filter_reset_trigger;      /* 5 */
    /* Arithmetic of the solve: 0 = fp64 (the reference's double, the default); 1 = fp32
     * (BASELINE configs[2]; differential drive only): iterate, multipliers and Newton systems
     * in float -- state a tolerance a float iterate can meet (tol ~1e-5 instead of 1e-8;
     * tiny_step_tol 10 FLT_EPSILON).  Inputs and outputs stay double.
     * Two phases (precision 1, no_restoration 0): the fp32 solver on the whole batch with these
     * params' options, then the fp64 solver with the reference's Ipopt options (the 3.12
     * defaults of the fields above; max_cpu_time and the problem parameters are kept) on the
     * whole batch again -- from the fp32 iterate, multipliers and barrier parameter where the
     * fp32 solve converged (status 1 or 4; diag[:, 2] = 4), from the start where it did not (its
     * line search failed where Ipopt would enter the restoration phase, a tiny step, the
     * iteration limit; diag[:, 2] = 3, bitwise the fp64 solver's result).  The outputs are the
     * fp64 phase's; iters counts both phases' iterations for a continued row, the fp64 solve's
     * for a row solved from the start.  Batches of more than 2,048 (solved in expected-longest-
     * first order): the B / 1024 problems ranked longest are solved by the fp64 solver from the
     * start (diag[:, 2] = 3) while the fp32 phase runs the others.  Which rows form this head
     * depends on the batch (its size and the other rows' ranks), so re-batching or sharding the
     * same problems can move a row between the head (the fp64 solve from the start) and the fp32
     * path (the fp64 continuation of its fp32 iterate); every other row's result, and every
     * result of the fp64 configuration, is independent of the batch. */
    int32_t precision;
    /* 0 (default): Ipopt's feasibility-restoration phase where the line search fails (fp32:
     * the two phases above); 1: stop there with RESTORATION_FAILURE (9) instead, and for
     * precision 1 the fp32 phase alone (its ending kept).  Occupies the struct's padding:
     * sizeof(mpcg_params) is unchanged. */
    int32_t no_restoration;
} mpcg_params;

typedef struct mpcg_handle mpcg_handle;

int mpcg_abi_version(void);
/* Hash of the sources the library was built from (mpc_ros_amd/build.py source_hash()). */
const char* mpcg_build_id(void);
const char* mpcg_last_error(void);

/* Defaults of an MPC object before LoadParams: MPC::MPC() (mpc_planner.cpp:223-241)
 * + FG_eval constructor (:42-68). */
int mpcg_params_default(mpcg_params* p);
/* Defaults the move_base plugin loads (mpc_ros/cfg/MPCPlanner.cfg:22-37, DT 0.1). */
int mpcg_params_plugin_default(mpcg_params* p);
/* One LoadParams map entry: key is one of the 15 reference keys, or one of the
 * extension keys MODEL (0 differential drive, 1 kinematic bicycle) and LF (wheelbase).
 * Returns 0 if applied, 1 if the key is unknown (ignored, as LoadParams ignores it). */
int mpcg_params_set(mpcg_params* p, const char* key, double value);
/* Validate a parameter set (steps >= 2, dt > 0, bounds > 0, weights >= 0). */
int mpcg_params_check(const mpcg_params* p);

/* Handle bound to one GPU (HIP device ordinal). */
int mpcg_create(int device, mpcg_handle** out);
void mpcg_destroy(mpcg_handle* h);
int mpcg_set_params(mpcg_handle* h, const mpcg_params* p);
int mpcg_get_params(const mpcg_handle* h, mpcg_params* p);
/* Device workspace for B problems (bytes): 4 slots per wavefront the GPU holds resident
 * (not per problem: the rare solver paths' copies), the park area of problems that enter the
 * restoration phase (max(256, B/128) entries, at most B; each holds the problem's state and
 * the restoration phase's records), the park-area overflow list (8 B per problem where the
 * area can overflow), and the solve-order buffers (B > 2048); reserve it ahead of graph
 * capture (a solve that must grow it allocates and synchronises the device). */
size_t mpcg_workspace_bytes(const mpcg_params* p, int64_t B);
/* The same for a handle: its parameters, its park capacity (mpcg_set_park_capacity) and the XCD
 * count of its device (the slot partitions) -- what mpcg_reserve(h, B) allocates. */
size_t mpcg_handle_workspace_bytes(const mpcg_handle* h, int64_t B);
int mpcg_reserve(mpcg_handle* h, int64_t B);
/* Park-area entries of the handle's solves (0 = the default max(256, B/128)).  A problem that
 * enters the restoration phase while every entry is taken goes to an overflow list and is
 * solved again from the start after the batch (the same iterates, diag[:, 2] = 2): results do
 * not depend on the capacity, only the tail does.  A tuning and test knob.  Set it before
 * mpcg_reserve: a larger capacity grows the workspace, and the next solve would otherwise
 * allocate it (with a device synchronisation -- not during graph capture). */
int mpcg_set_park_capacity(mpcg_handle* h, int64_t cap);
/* The solver kernel instance the handle's last solve launched, "k_solve_wide<model, split,
 * type, stage blocks, default options, waves per SIMD>" ("" before the first solve). */
const char* mpcg_last_kernel(const mpcg_handle* h);
/* 1 if the handle's last solve ran its problems in expected-longest-first order (batches of
 * B > 2048: a radix sort of the path curvature before the batch kernel), 0 otherwise. */
int mpcg_last_solve_order(const mpcg_handle* h);

/* Batched solve, host buffers, synchronous (copies in, solves, copies out).
 *   state  [B][6]  x, y, theta, v, cte, etheta   (MPC::Solve `state`)
 *   coeffs [B][4]  c0..c3                        (MPC::Solve `coeffs`)
 *   u0     [B][2]  omega_0, a_0                  (MPC::Solve return value)
 *   traj   [B][3][N] mpc_x | mpc_y | mpc_theta   (MPC::mpc_x/mpc_y/mpc_theta) or NULL
 *   status [B] or NULL, obj [B] or NULL, iters [B] or NULL */
int mpcg_solve(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, double* u0,
               double* traj, int32_t* status, double* obj, int32_t* iters);

/* Batched solve on device-resident buffers (same layouts), queued on `stream` (a
 * hipStream_t; NULL = the null stream, as everywhere in HIP) without any host
 * synchronisation: the solve-order sort (B > 2048), a workspace reset, the batch kernel and
 * the restoration phase's resume kernels; work forked onto the handle's own streams (resume
 * workers, the fp32 configuration's head) is joined back into `stream` by events, so the
 * sequence can be captured in a HIP graph.  Synchronise the stream before reading the outputs
 * on the host.  No allocation if mpcg_reserve(h, B) was called. */
int mpcg_solve_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, double* d_u0,
                      double* d_traj, int32_t* d_status, double* d_obj, int32_t* d_iters, void* stream);

/* mpcg_solve / mpcg_solve_device with per-problem solver diagnostics diag [B][4] (int32,
 * may be NULL): restoration phases entered, filter entries dropped beyond its capacity
 * (filter_cap in LDS plus 448 in the workspace; Ipopt's filter is unbounded, so any nonzero
 * value marks a solve that may differ from Ipopt's), 1 if the problem was continued by the
 * parked-problem kernel (2 if it was solved again after a park-area overflow; precision 1: 4 if
 * the fp64 phase continued from the fp32 iterate, 3 if it solved the problem from the start;
 * 0 otherwise), the
 * most filter entries held at once (the original problem). */
int mpcg_solve_ex(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, double* u0, double* traj,
                  int32_t* status, double* obj, int32_t* iters, int32_t* diag);
int mpcg_solve_device_ex(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, double* d_u0,
                         double* d_traj, int32_t* d_status, double* d_obj, int32_t* d_iters, int32_t* d_diag,
                         void* stream);

/* Multi-GPU batched solves from one process, host buffers as
 * mpcg_solve: the B problems are split into ngpu contiguous shards (the first B % ngpu
 * GPUs take one more), solved on devices[r] with the given parameters, and the results are
 * gathered to devices[0] by grouped RCCL send/recv (one message per output array and GPU,
 * point-to-point over xGMI), then copied to the host.
 *
 * mpcg_multi: a persistent context for a serving loop -- the RCCL communicator
 * (ncclCommInitAll), a handle, stream and device buffers per GPU, and each handle's solver
 * workspace reserved for the largest shard of B_max problems, all created once by
 * mpcg_multi_create; mpcg_multi_solve then allocates nothing (batches of B <= B_max; the
 * parameters are the context's).  A failure inside the gather group aborts the communicators
 * and marks the context broken (later solves return -4; destroy and create it again).
 * mpcg_solve_multi = create + solve + destroy for one batch.  Returns 0, or < 0 with
 * mpcg_last_error() set (-1 arguments, -2 HIP, -3 device ordinal, -4 RCCL). */
typedef struct mpcg_multi mpcg_multi;
int mpcg_multi_create(int ngpu, const int* devices, const mpcg_params* params, int64_t B_max, mpcg_multi** out);
int mpcg_multi_solve(mpcg_multi* m, int64_t B, const double* state, const double* coeffs, double* u0, double* traj,
                     int32_t* status, double* obj, int32_t* iters);
void mpcg_multi_destroy(mpcg_multi* m);
int mpcg_solve_multi(int ngpu, const int* devices, const mpcg_params* params, int64_t B, const double* state,
                     const double* coeffs, double* u0, double* traj, int32_t* status, double* obj, int32_t* iters);

/* mpcg_solve_multi's arithmetic, pure functions (no GPU):
 * mpcg_shard_range: GPU r of ngpu solves problems [start, start + count) -- contiguous,
 *   the first B % ngpu GPUs one more, empty shards when B < ngpu.
 * mpcg_multi_gather_plan: the MPCG_GATHER_ARRAYS messages GPU r sends to devices[0]
 *   (u0, traj, obj, status, iters): byte offsets in its own output buffer and in the root's
 *   gathered buffer of mpcg_multi_out_bytes(B, N) bytes, and sizes (count x 32 + 24 N bytes
 *   in all; 0 for an empty shard).  For r = 0 src_offset == dst_offset: the root solves in
 *   place and sends nothing. */
#define MPCG_GATHER_ARRAYS 5
typedef struct mpcg_xfer {
    size_t src_offset, dst_offset, bytes;
} mpcg_xfer;
int mpcg_shard_range(int64_t B, int ngpu, int r, int64_t* start, int64_t* count);
int mpcg_multi_gather_plan(int64_t B, int32_t N, int ngpu, int r, mpcg_xfer* xfers);
size_t mpcg_multi_out_bytes(int64_t B, int32_t N);
/* mpcg_multi_buffer_bytes: the device buffers a context for batches of up to B_max holds on
 * GPU r (inputs of the largest shard; outputs of that shard, or on the root the gathered
 * outputs of B_max problems), besides the handle's solver workspace (mpcg_workspace_bytes of
 * the largest shard).  0 for invalid arguments. */
size_t mpcg_multi_buffer_bytes(int64_t B_max, int32_t N, int ngpu, int r);

/* Tracking::findBestPath's preprocessing (mpc_ros/src/driving_state.cpp:175-256) on the
 * device for B robots: waypoints to the vehicle frame, cubic polyfit (Householder QR),
 * cte, heading error from the first int(0.3 M) waypoint increments, delay-mode
 * prediction.  M waypoints per robot, the same for the batch: M >= 4 (polyfit asserts
 * order 3 <= M - 1, driving_state.cpp:286); plans beyond 64 waypoints take a handle-owned
 * device scratch of 48 M B bytes (used stream-ordered).
 *   pose [B][3]  x, y, yaw                       (global_pose)
 *   vel  [B][3]  v feedback, previous w, previous throttle (feedback_vel.linear.x, _w, _throttle)
 *   plan [B][M][2] waypoints x, y                (ref_plan)
 *   state [B][6], coeffs [B][4]                  the arguments of MPC::Solve (outputs)
 * dt = the handle's DT.  Queued on `stream`; no solve. */
int mpcg_preprocess_device(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                           const double* d_plan, int32_t delay_mode, double* d_state, double* d_coeffs,
                           void* stream);

/* One control tick of Tracking::findBestPath for B robots: preprocessing, the solve,
 * and the post-processing of driving_state.cpp:262-269.
 *   cmd [B][3]  speed = min(v + throttle dt, REF_V), w = w0, throttle = a0
 *   traj [B][3][N], status [B]: as mpcg_solve_device (may be NULL).
 * Intermediate state/coeffs/controls live in handle-owned device buffers. */
int mpcg_track_device(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                      const double* d_plan, int32_t delay_mode, double* d_cmd, double* d_traj, int32_t* d_status,
                      void* stream);

/* ---- Per-problem parameters: one batch, one parameter row per robot ----
 * In the reference every robot owns its parameter map: Tracking::deceleration rewrites REF_V
 * from the distance to the robot's own goal before every solve (driving_state.cpp:121-141), and
 * dynamic_reconfigure sets weights and limits per robot.  A row holds the per-problem fields of
 * one robot as MPCG_PP_FIELDS doubles (128 bytes, one line per problem) in the order of the
 * MPCG_PP_* indices; rows [B][16].  STEPS, MODEL, the precision and every Ipopt option stay the
 * handle's, the same for the whole batch: they fix the kernel instance and the LDS layout. */
#define MPCG_PP_DT 0
#define MPCG_PP_REF_CTE 1
#define MPCG_PP_REF_ETHETA 2
#define MPCG_PP_REF_V 3
#define MPCG_PP_W_CTE 4
#define MPCG_PP_W_EPSI 5
#define MPCG_PP_W_V 6
#define MPCG_PP_W_ANGVEL 7
#define MPCG_PP_W_A 8
#define MPCG_PP_W_DANGVEL 9
#define MPCG_PP_W_DA 10
#define MPCG_PP_ANGVEL 11
#define MPCG_PP_MAXTHR 12
#define MPCG_PP_BOUND 13
#define MPCG_PP_LF 14
#define MPCG_PP_RESERVED 15 /* written as 0, not read */
#define MPCG_PP_FIELDS 16
/* B rows, each the per-problem fields of *p (pure host function). */
int mpcg_pparams_fill(const mpcg_params* p, int64_t B, double* rows);
/* The domains of mpcg_params_check on B rows (pure host function): every value finite,
 * DT, ANGVEL, MAXTHR, BOUND > 0, the weights >= 0, LF > 0 for model 1.  Returns 0, or -1 with
 * the first offending row in *bad_row (may be NULL) and in mpcg_last_error(). */
int mpcg_pparams_check(const double* rows, int64_t B, int32_t model, int64_t* bad_row);
/* mpcg_solve_ex with a parameter row per problem (host buffers, synchronous).  The rows are
 * checked with mpcg_pparams_check first: a bad row returns -1 and nothing is solved.  The
 * handle's own per-problem fields are ignored. */
int mpcg_solve_pp(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                  double* u0, double* traj, int32_t* status, double* obj, int32_t* iters, int32_t* diag);
/* mpcg_solve_device_ex with a parameter row per problem, d_pparams [B][16] on the device: queued
 * exactly as mpcg_solve_device_ex (the sort for B > 2048, the workspace reset, the batch kernel,
 * the resume workers, the drain and the overflow launch; no allocation after mpcg_reserve;
 * capturable in a HIP graph -- a replay reads the rows as they are then).  The rows are read by
 * the batch kernel and again by the resume kernels (problem p always reads row p, also in an
 * ordered launch): keep them unchanged until the stream has passed the solve.  mpcg_last_kernel
 * names the per-problem instance, "k_solve_wide_pp<...>".
 * Rows are validated on the device, before the solve (the domains of mpcg_pparams_check): a
 * problem with an invalid row ends with status 13 (internal_error), iters 0, u0 = 0, traj = 0,
 * obj = NaN and diag = 0.  Nothing traps -- a caller's bad data does not cost the HIP context --
 * and the other problems are unaffected.
 * precision 1 is refused (-1): the two-phase fp32 configuration would need per-problem
 * instances of its fp64 phase and head as well. */
int mpcg_solve_device_pp(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                         const double* d_pparams, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                         int32_t* d_iters, int32_t* d_diag, void* stream);
/* Tracking::deceleration's rule (driving_state.cpp:121-141) as a pure host function: the REF_V
 * of a robot at distance dist from its goal, moving at v.  The reference's quirk is kept: the
 * first branch sets max_speed, not speed.
 *     if dist <= v^2 / max_throttle:
 *         speed = max_throttle * dist
 *         speed > ref_v: max_speed;  speed < min_speed: min_speed;  otherwise speed
 *     otherwise ref_v, unchanged. */
double mpcg_decelerate(double dist, double v, double max_throttle, double max_speed, double min_speed, double ref_v);
/* One control tick of Tracking::mpcComputeVelocityCommands for B robots (driving_state.cpp:
 * 105-119): deceleration, then mpcg_track_device's preprocessing (the handle's DT), the solve
 * with a parameter row per robot, and the post-processing per robot.
 *   goal  [B][2]  the robot's goal x, y
 *   ref_v [B]     in/out: the robot's REF_V, rewritten by mpcg_decelerate's rule from
 *                 dist = hypot(pose.xy - goal) (correctly rounded) and v = vel[:, 0]; the value
 *                 persists between ticks as the reference's map entry does -- pass it back in
 *   max_speed, min_speed: the reference's 0.7 and 0.05 (driving_state.cpp:26, :29)
 *   cmd   [B][3]  speed = min(v + throttle dt, ref_v[b]), w = w0, throttle = a0
 * The rule's max_throttle is the handle's MAXTHR, at least 0.1 as the reference clamps its own
 * copy (driving_state.cpp:63; the solve's bound stays the handle's MAXTHR).  Each robot's row is
 * the handle's parameters with REF_V = ref_v[b], in a handle-owned device buffer used
 * stream-ordered like the other intermediates.  precision 1 is refused as in
 * mpcg_solve_device_pp. */
int mpcg_track_device_goal(mpcg_handle* h, int64_t B, int32_t M, const double* d_pose, const double* d_vel,
                           const double* d_plan, const double* d_goal, double* d_ref_v, double max_speed,
                           double min_speed, int32_t delay_mode, double* d_cmd, double* d_traj, int32_t* d_status,
                           void* stream);

/* ---- Closed loop on the device: plan window, a waypoint count per robot, K-tick rollout ----
 * What the reference does between two solves -- MPCPlannerROS::getCutOffPlan and downSamplePlan
 * (mpc_ros/src/mpc_planner_ros.cpp:266-291, :365-391) before findBestPath, and the command fed
 * back -- for B robots on the device, so that B robots x K ticks are one enqueue on a stream.
 *
 * The window rule, on a course of G waypoints [G][2] addressed by index instead of erased, from
 * the robot's cursor c (0 <= c < G) and its pose (x, y):
 *   cut:    d_prev = 10e5 (the reference's literal); for i from c, while i < G and not
 *           d_prev < d_i (d_i = dx dx + dy dy, dx = x - wp_i.x, as the reference evaluates it):
 *           d_prev = d_i, ++i.  The window starts at start = i, the first waypoint whose distance
 *           increases -- the nearest one itself is erased, as in the reference; a robot farther
 *           than 1000 m from waypoint c erases nothing.  The new cursor is max(c, start - 1).
 *   window: W = min(window_wp, G - start) waypoints from start.  window_wp (>= 1) stands in for
 *           the costmap-limited local plan (LocalPlannerUtil::getLocalPlan).
 *   sample: indices start, start + stride, ... < start + W, then start + W - 1 once more, always
 *           (the reference pushes back() unconditionally: the last waypoint appears twice where
 *           W - 1 is a multiple of stride).  stride (>= 1) is the reference's _downSampling,
 *           int(path_length / 10 / hypot(wp1 - wp0)).
 *           count = ceil(W / stride) + 1, or 0 if W = 0; at most
 *           Mmax = ceil(window_wp / stride) + 1 = mpcg_plan_window_mmax(window_wp, stride). */
int32_t mpcg_plan_window_mmax(int32_t window_wp, int32_t stride); /* -1: window_wp or stride < 1, or beyond int32 */
/* One robot, pure host function (the code the kernel runs).  plan [Mmax][2]: the count sampled
 * waypoints, copied bit for bit, then zeros.  new_cursor, start, count: outputs (each may be
 * NULL).  Returns 0, or -1 (course or plan NULL, G < 1, cursor outside [0, G), window_wp < 1,
 * stride < 1) with nothing written. */
int mpcg_plan_window(const double* course, int32_t G, int32_t cursor, double x, double y, int32_t window_wp,
                     int32_t stride, int32_t* new_cursor, int32_t* start, int32_t* count, double* plan);
/* B robots on the device, one per lane.  Courses are shared: courses [C][Gmax][2], course_len [C]
 * (1 <= len <= Gmax), course_of [B] the robot's course.
 *   pose   [B][3]        x, y, yaw (yaw is not read)
 *   cursor [B] int32     in/out
 *   plan   [B][Mmax][2]  rows past the robot's count are written as 0
 *   count  [B] int32
 * A robot whose course_of, course length or cursor is out of range reads no course: count 0,
 * cursor unchanged.  Nothing traps.  Refused (-1): window_wp < 1, stride < 1, C < 1, Gmax < 1,
 * Mmax > 64 (the preprocessing below keeps a robot's plan in registers).  Queued on `stream`. */
int mpcg_plan_window_device(mpcg_handle* h, int64_t B, const double* d_courses, const int32_t* d_course_len,
                            const int32_t* d_course_of, int32_t C, int32_t Gmax, const double* d_pose,
                            int32_t window_wp, int32_t stride, int32_t* d_cursor, double* d_plan, int32_t* d_count,
                            void* stream);
/* mpcg_preprocess_device with a waypoint count per robot: plan [B][Mmax][2] (1 <= Mmax <= 64),
 * count [B] int32; robot p is fitted to its first count[p] rows, and the heading from the first
 * int(0.3 count[p]) increments and everything after it use its own count -- for a uniform count
 * = Mmax, bitwise mpcg_preprocess_device's result.  A robot with count < 4 (polyfit asserts order
 * 3 <= M - 1) or count > Mmax is not fitted: its state and coeffs are written as 0 (the rollout
 * marks such a robot done). */
int mpcg_preprocess_device_n(mpcg_handle* h, int64_t B, int32_t Mmax, const double* d_pose, const double* d_vel,
                             const double* d_plan, const int32_t* d_count, int32_t delay_mode, double* d_state,
                             double* d_coeffs, void* stream);
/* The logs of a rollout, each may be NULL; row k holds what tick k saw and what it returned. */
typedef struct mpcg_rollout_logs {
    double* pose;    /* [K][B][3] the pose the tick started from */
    double* vel;     /* [K][B][3] the feedback it started from */
    double* cmd;     /* [K][B][3] the command it returned (0 for a done robot) */
    int32_t* cursor; /* [K][B] the cursor after the tick's cut */
    int32_t* start;  /* [K][B] the window's first waypoint */
    int32_t* count;  /* [K][B] its sampled waypoints */
    int32_t* status; /* [K][B] the solve's status (13 for a done robot) */
    int32_t* iters;  /* [K][B] the solve's iterations (0 for a done robot) */
    double* ref_v;   /* [K][B] REF_V after the tick's deceleration */
} mpcg_rollout_logs;
/* K control ticks of B robots, queued on `stream` one after another.  Per tick:
 *   1. the plan window (mpcg_plan_window_device's kernel, Mmax from window_wp and stride);
 *   2. Tracking::deceleration towards the robot's goal, its course's last waypoint
 *      (mpcg_track_device_goal's rule and correctly rounded distance), for every robot with a
 *      course, done or not;
 *   3. the preprocessing with the robot's own count (mpcg_preprocess_device_n's kernel);
 *   4. the solve with each robot's row and the post-processing, as mpcg_track_device_goal;
 *   5. if `integrate`: the unicycle of closed_loop.run over one control period (the handle's DT),
 *      x += speed cos(yaw) dt, y += speed sin(yaw) dt, yaw = atan2(sin, cos)(yaw + w dt), and
 *      vel = (speed, w, throttle).  integrate = 0 leaves pose and vel alone: with K = 1 this is
 *      the real robot's tick from a global plan, its command in logs->cmd.
 * A robot is done at the first tick where its window has fewer than 4 waypoints (a robot without
 * a course included) or its distance to its goal is <= goal_tol: done[b] takes that tick's index
 * within this call + 1 (0 = running; a robot that comes in done stays as it is).  From that tick
 * on its command is 0, with `integrate` its vel is 0 and its pose frozen, and it costs no solver
 * iterations: its parameter row is invalid (DT = 0), so the solve's row validation ends it at
 * iteration 0 with status 13 (mpcg_solve_device_pp).
 *   pose [B][3], vel [B][3], cursor [B] int32, ref_v [B], done [B] int32: in/out -- the state a
 *   later call carries on from (K ticks in one call equal K calls of one tick).
 * No host synchronisation; no allocation once the handle's buffers exist (the window's plan and
 * counts, the track buffers and rows; the solver workspace after mpcg_reserve): call it once
 * before a graph capture.  Refused (-1): K < 1, window_wp < 1, stride < 1, Mmax > 64, C < 1,
 * Gmax < 1, precision 1 (as mpcg_track_device_goal). */
int mpcg_rollout_device(mpcg_handle* h, int64_t B, int32_t K, const double* d_courses, const int32_t* d_course_len,
                        const int32_t* d_course_of, int32_t C, int32_t Gmax, int32_t window_wp, int32_t stride,
                        double goal_tol, double max_speed, double min_speed, int32_t delay_mode, int32_t integrate,
                        double* d_pose, double* d_vel, int32_t* d_cursor, double* d_ref_v, int32_t* d_done,
                        const mpcg_rollout_logs* logs, void* stream);

/* ---- The full solution and its certificate ----
 * What CppAD::ipopt::solve_result carries beyond the first control: the primal point and every
 * multiplier of the ORIGINAL, unscaled NLP, in the reference's vars order (mpc_planner.cpp:252-259)
 * and FG_eval's row order (fg[1 + i]).  One problem's record, mpcg_solution_elems(N) =
 * 3 (8N - 2) + 6N doubles:
 *   x      [8N-2]  x(N) | y(N) | theta(N) | v(N) | cte(N) | etheta(N) | omega(N-1) | a(N-1)
 *   zl     [8N-2]  lower-bound multipliers (>= 0), same order
 *   zu     [8N-2]  upper-bound multipliers (>= 0), same order
 *   lambda [6N]    constraint multipliers, row s N + k (s: x y theta v cte etheta; k = 0 the
 *                  initial-state row, k >= 1 the dynamics defect of step k - 1)
 * Ipopt's / CppAD's convention: the Lagrangian is sigma f + sum lambda_i g_i, stationarity reads
 * grad f + J^T lambda - zl + zu = 0.  The solver's objective and row scaling is undone (Ipopt's
 * finalize_solution).  x is the point u0 and traj publish (honor_original_bounds applied):
 * x[0..N), x[N..2N), x[2N..3N) equal traj and x[6N], x[7N-1] equal u0 bit for bit.
 * solve_result.g is not in the record: at a returned point it is the constraint bounds (state[s]
 * for row s N, 0 elsewhere) to within the violation the certificate's column 1 reports.
 * Every ending writes the record: a status other than 1 or 4 the iterate the solve ended with
 * (what Ipopt hands to finalize_solution), an invalid parameter row (status 13) zeros.  Row p of
 * sol is problem p's, whatever the solve order. */
int64_t mpcg_solution_elems(int32_t N);
/* byte offsets of the four parts within one problem's record */
#define MPCG_SOL_X_OFFSET(N) ((size_t)0)
#define MPCG_SOL_ZL_OFFSET(N) ((size_t)(8 * (N) - 2) * sizeof(double))
#define MPCG_SOL_ZU_OFFSET(N) ((size_t)2 * (8 * (N) - 2) * sizeof(double))
#define MPCG_SOL_LAMBDA_OFFSET(N) ((size_t)3 * (8 * (N) - 2) * sizeof(double))
/* mpcg_solve_ex / mpcg_solve_device_ex with the records sol [B][mpcg_solution_elems(N)] (required)
 * and a parameter row per problem, pparams [B][16] (NULL: the handle's parameters; otherwise as
 * mpcg_solve_pp / mpcg_solve_device_pp).  The iterates, and with them u0, traj, status, iters and
 * obj, are bitwise those of the call without sol.  The device call is queued on `stream` like its
 * twin (no allocation after mpcg_reserve; capturable).  Refused (-1) before anything is launched:
 * a NULL sol; precision 1 with no_restoration 1 (the fp32 phase alone has no fp64 ending to
 * report -- with no_restoration 0 the record is the fp64 phase's); precision 1 with rows.
 * mpcg_multi_* is unchanged: the multi-GPU gather does not carry the record. */
int mpcg_solve_sol(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                   double* u0, double* traj, int32_t* status, double* obj, int32_t* iters, int32_t* diag, double* sol);
int mpcg_solve_device_sol(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                          const double* d_pparams, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                          int32_t* d_iters, int32_t* d_diag, double* d_sol, void* stream);
/* ---- Start point in ----
 * The solve of mpcg_solve_sol / mpcg_solve_device_sol started from a solution record per problem:
 * start [B][mpcg_solution_elems(N)] in the layout above (required), start_mode [B] (required), one
 * of
 *   MPCG_START_COLD    the solve of mpcg_solve_device_sol: same iterates, bitwise outputs; the
 *                      record is not read.
 *   MPCG_START_PRIMAL  what the reference computes when the record's x is passed as
 *                      CppAD::ipopt::solve's xi.  Only x is read.  The objective scale and the row
 *                      scales come from the gradient and the Jacobian at x as given; x is then
 *                      pushed inside the relaxed bounds (bound_push = bound_frac = 0.01); z = 1,
 *                      least-squares lambda, mu_init.
 *   MPCG_START_FULL    Ipopt's warm_start_init_point yes with its 3.12 defaults: the cold solve's
 *                      scaling; x pushed inside the relaxed bounds by warm_start_bound_push =
 *                      warm_start_bound_frac = 1e-3; zl, zu from the record, floored at
 *                      warm_start_mult_bound_push = 1e-3; lambda from the record, 0 where it
 *                      exceeds warm_start_mult_init_max = 1e6 in magnitude; the barrier parameter
 *                      mu0[b] (mu0 NULL: the handle's mu_init; read in this mode only); a fresh
 *                      filter and line search, the iteration count from 0.
 * start_used [B] (may be NULL) receives the mode that ran: 0, 1 or 2; -1 when the start has a
 * non-finite entry in a part the mode reads, a negative zl / zu or a mu0 that is not positive and
 * finite (FULL), or the mode is none of the three; -2 (PRIMAL) when a Jacobian entry at x exceeds
 * 100 (a row scale other than 1).  A negative value means the problem was solved cold, bitwise the
 * cold result; nothing traps on a caller's start.  A problem whose parameter row is invalid
 * (status 13) reports 0.
 * sol may be NULL, and sol may alias start (the in-place loop): a problem's start is read before
 * anything of its record is written, by whichever kernel ends up solving it.
 * The device call is queued on `stream` like mpcg_solve_device_sol: it does not synchronise, does
 * not allocate after mpcg_reserve, and can be captured in a HIP graph.  d_start, d_start_mode and
 * d_mu0 are read again for a park-overflow re-solve: keep them unchanged until the stream has
 * passed the solve, as d_pparams (d_sol aliasing d_start is the exception the solver orders
 * itself).  Results do not depend on the park capacity or the solve order.
 * Refused (-1) before anything is launched: a NULL start or start_mode; precision 1.
 * mpcg_last_kernel reports the k_start_wide instance.  mpcg_multi_* and the ticks are unchanged;
 * the rollout started from each robot's previous record is mpcg_rollout_device_start below. */
#define MPCG_START_COLD 0
#define MPCG_START_PRIMAL 1
#define MPCG_START_FULL 2
int mpcg_solve_start(mpcg_handle* h, int64_t B, const double* state, const double* coeffs, const double* pparams,
                     const double* start, const int32_t* start_mode, const double* mu0, double* u0, double* traj,
                     int32_t* status, double* obj, int32_t* iters, int32_t* diag, double* sol, int32_t* start_used);
int mpcg_solve_device_start(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                            const double* d_pparams, const double* d_start, const int32_t* d_start_mode,
                            const double* d_mu0, double* d_u0, double* d_traj, int32_t* d_status, double* d_obj,
                            int32_t* d_iters, int32_t* d_diag, double* d_sol, int32_t* d_start_used, void* stream);
/* The KKT certificate of B records, from the NLP alone (the reference's FG_eval and MPC::Solve's
 * original, unrelaxed bounds; no solver code, no scaling): cert [B][4], all unscaled,
 *   0  || grad f + J^T lambda - zl + zu ||_inf
 *   1  max(|| g(x) - g_bound ||_inf, the largest bound violation of x)
 *   2  max over the variables of max(|(x - xl) zl|, |(xu - x) zu|)
 *   3  f(x)
 * pparams: a parameter row per problem or NULL (then *p / the handle's parameters); a problem
 * whose row is outside mpcg_pparams_check's domains gets NaN in all four columns, nothing traps.
 * mpcg_kkt: host arrays, no GPU and no handle (the code the kernel runs per stage, in a loop).
 * mpcg_kkt_device: device arrays, one problem per wavefront, queued on `stream`; no allocation,
 * capturable.  Host and device agree to rounding (sin / cos and the order of the objective's sum). */
int mpcg_kkt(const mpcg_params* p, int64_t B, const double* state, const double* coeffs, const double* pparams,
             const double* sol, double* cert);
int mpcg_kkt_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, const double* d_pparams,
                    const double* d_sol, double* d_cert, void* stream);

/* ---- A record carried to the next tick ----
 * findBestPath poses every problem in the robot's own frame at that tick, so the record of tick t
 * is, as a start for tick t + 1, one stage late and rotated and translated by the robot's motion.
 * The shift rule (mpc_ros_amd/csrc/mpcg_shift.h) makes it the start of the next problem; it is by
 * exactly one stage, so it assumes a control period equal to DT.
 *   motion [B][3] = (mx, my, mpsi): the new frame's origin and heading, expressed in the old frame.
 *   With c = cos(mpsi), s = sin(mpsi): a point maps as x' = c (x - mx) + s (y - my), y' =
 *   -s (x - mx) + c (y - my); a heading as theta' = theta - mpsi (not wrapped: the NLP's theta is a
 *   free variable); a vector by the rotation alone.
 * Output record o from source r, N stages:
 *   states s, k = 0..N-2   o.x[sN + k] = r.x[sN + k + 1], x y theta through the maps; then
 *                          o.x[sN + 0] = state[s], so the new initial-state rows hold exactly
 *   controls               o.x[6N + k] = r.x[6N + k + 1] for k = 0..N-3, the last one held
 *                          (o.x[7N - 2] = r.x[7N - 2]); the same for a
 *   terminal state         one step of the model from o's stage N-2 under o's control N-2, with
 *                          the new coeffs and parameter row: the six rows of the last dynamics
 *                          step have zero defect as mpcg_kkt evaluates them
 *   zl, zu                 x's index map, no frame map, no stage-0 overwrite; stage N-1 held
 *   lambda                 o.lambda[sN + k] = r.lambda[sN + k + 1] for k = 0..N-2, the last row
 *                          held; the (x, y) row pair of every k rotated as a vector
 * The rule does not validate its input: non-finite entries pass through, and mpcg_solve_start
 * turns such a start into a cold solve (start_used -1).
 * state, coeffs, pparams: the NEW problem's (pparams NULL: *p / the handle's parameters).
 * mask [B] int32 or NULL: where it is 0 the record is copied unchanged.  sol_out may alias sol_in.
 * mpcg_shift_solution: host arrays, no GPU and no handle.  mpcg_shift_solution_device: device
 * arrays, one problem per wavefront, queued on `stream`; no allocation, no synchronisation, nothing
 * traps; capturable.  Host and device agree to rounding (sin / cos). */
int mpcg_shift_solution(const mpcg_params* p, int64_t B, const double* state, const double* coeffs,
                        const double* pparams, const double* motion, const int32_t* mask, const double* sol_in,
                        double* sol_out);
int mpcg_shift_solution_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs,
                               const double* d_pparams, const double* d_motion, const int32_t* d_mask,
                               const double* d_sol_in, double* d_sol_out, void* stream);
/* mpcg_rollout_device with every tick started from the robot's own previous solution.  start_mode:
 * MPCG_START_COLD or MPCG_START_FULL, the same for all robots (MPCG_START_PRIMAL is refused: a
 * PRIMAL-started solve inside the rollout's kernel sequence did not repeat bit for bit from call to
 * call, DESIGN.md "Carry to the next tick"; mpcg_shift_solution_device and mpcg_solve_device_start
 * compose a PRIMAL tick); mu0: FULL's barrier parameter (read in FULL mode only).  The carry is the caller's, in/out like pose and done (zeros before the first tick):
 *   carry_sol  [B][mpcg_solution_elems(N)]  the robot's last record
 *   carry_pose [B][3]                       the pose whose frame that record is in
 *   carry_ok   [B] int32                    1: the record is a solution (status 1 or 4)
 *   log_start_used [K][B] int32 or NULL     the mode that ran (mpcg_solve_device_start's start_used)
 * Per tick, after the preprocessing: robot b uses its record if carry_ok[b] != 0, done[b] == 0 and
 * start_mode != COLD -- its motion from carry_pose[b] = (X0, Y0, psi0) to the tick's pose (X1, Y1,
 * psi1) is mx = cos psi0 dX + sin psi0 dY, my = -sin psi0 dX + cos psi0 dY, mpsi = atan2(sin(psi1 -
 * psi0), cos(psi1 - psi0)), the record is shifted in place and its mode is start_mode; every other
 * robot runs COLD.  carry_pose[b] takes the tick's pose of a running robot.  The solve is
 * mpcg_solve_device_start's with start = sol = carry_sol and the robots' parameter rows.  Afterwards
 * carry_ok[b] = (done[b] == 0 and status[b] is 1 or 4).
 * K ticks in one call equal K calls of one tick bitwise, the carry included; integrate = 0, K = 1 is
 * the real robot's warm tick.  With start_mode COLD every log and every state array is bitwise
 * mpcg_rollout_device's, and the carry holds what mpcg_solve_device_sol would write.
 * mpcg_last_kernel reports the k_start_wide instance.  Refused (-1) before the first launch:
 * mpcg_rollout_device's refusals; a NULL carry pointer; PRIMAL or an unknown mode; a mu0 that is not
 * positive and finite in FULL mode. */
int mpcg_rollout_device_start(mpcg_handle* h, int64_t B, int32_t K, const double* d_courses,
                              const int32_t* d_course_len, const int32_t* d_course_of, int32_t C, int32_t Gmax,
                              int32_t window_wp, int32_t stride, double goal_tol, double max_speed, double min_speed,
                              int32_t delay_mode, int32_t integrate, double* d_pose, double* d_vel, int32_t* d_cursor,
                              double* d_ref_v, int32_t* d_done, const mpcg_rollout_logs* logs, void* stream,
                              int32_t start_mode, double mu0, double* d_carry_sol, double* d_carry_pose,
                              int32_t* d_carry_ok, int32_t* d_log_start_used);

/* ---- Sensitivities of the solution ----
 * The first-order feedback law around a solution record: gain [B][2][10] (row-major) =
 * d(omega_0, a_0) / d(state[0..5], coeffs[0..3]), from the NLP and the record alone (no solver
 * code, no scaling).  With W the Hessian in x of f + sum lambda_i g_i at the record's x, J the
 * Jacobian of g, r_i = min(constr_viol_tol, bound_relax_factor max(1, |bound_i|)) the solver's
 * bound relaxation and Sigma = diag(zl_i / (x_i - (xl_i - r_i)) + zu_i / ((xu_i + r_i) - x_i))
 * (xl, xu MPC::Solve's original bounds), it solves for ten right-hand sides
 *     [ W + Sigma  J^T ] [ dx      ]   [ a_c ]
 *     [ J          0   ] [ dlambda ] = [ b_c ]
 *   c = 0..5, state component s: a = 0, b = the unit vector of row s N (the initial-state row);
 *   c = 6..9, coefficient c_i:   b[4N + k + 1] = x_k^i and a[x_k] = i x_k^(i-1) lambda[4N + k + 1]
 *                                for k = 0..N-2 (the polynomial enters the cte rows only)
 * by one backward Riccati sweep over the stages (the state augmented with the previous control)
 * and one forward sweep.  gain[r][c] = dx_c[6N] (r = 0) and dx_c[7N - 1] (r = 1).  No thresholding:
 * where u0 sits at its bound the row is about 1e-7, not exactly 0.  Meaningful where the solve
 * ended with status 1 or 4; the status is not looked at.
 *   dx   [B][10][8N-2] or NULL: the full primal columns in the record's variable order
 *   info [B] int32 or NULL:
 *     0  gain valid
 *     1  a stage's reduced control Hessian R + B^T P B was not positive definite: the KKT matrix
 *        does not have inertia (8N-2, 6N); gain and dx are NaN
 *     2  a parameter row outside mpcg_pparams_check's domains, a non-finite record entry or
 *        coefficient, or a slack <= 0 (x outside its relaxed bound); gain and dx are NaN
 * pparams: as in mpcg_kkt.  state is not read (the gain does not depend on the bound of the
 * initial-state rows); it is in the signature for symmetry with mpcg_kkt and may be NULL.
 * mpcg_sens: host arrays, no GPU and no handle (the kernel's code with the 64 lanes in a loop).
 * mpcg_sens_device: device arrays, one problem per wavefront, the work area in LDS at every
 * horizon (2 <= N <= 128), queued on `stream`; no solver state, no workspace, no atomics, no
 * allocation, capturable; nothing traps.  Host and device agree to rounding (sin / cos).
 * Refused (-1) before any launch: a NULL sol or gain; precision 1 with rows. */
#define MPCG_SENS_COLS 10
int mpcg_sens(const mpcg_params* p, int64_t B, const double* state, const double* coeffs, const double* pparams,
              const double* sol, double* gain, double* dx, int32_t* info);
int mpcg_sens_device(mpcg_handle* h, int64_t B, const double* d_state, const double* d_coeffs, const double* d_pparams,
                     const double* d_sol, double* d_gain, double* d_dx, int32_t* d_info, void* stream);
/* The correction without a solve (the advanced-step correction of a delay-mode prediction):
 * u[b] = clip(u0[b] + gain[b] [dstate[b]; dcoeffs[b]]) to +-ANGVEL, +-MAXTHR (the row's if pparams
 * is given; dcoeffs may be NULL = 0); a sum that is not finite (a NaN gain) gives u = u0.
 * u0, u [B][2], dstate [B][6], dcoeffs [B][4].  mpcg_sens_apply: the rule as a pure host function;
 * mpcg_sens_apply_device: one robot per lane, queued on `stream`, bitwise the host rule. */
int mpcg_sens_apply(const mpcg_params* p, int64_t B, const double* pparams, const double* gain, const double* u0,
                    const double* dstate, const double* dcoeffs, double* u);
int mpcg_sens_apply_device(mpcg_handle* h, int64_t B, const double* d_pparams, const double* d_gain, const double* d_u0,
                           const double* d_dstate, const double* d_dcoeffs, double* d_u, void* stream);

/* The benchmark's synthetic robots (the "infinity set", mpc_ros_amd/infinity.py) generated on
 * the device: robot start + i of the set (i < B) is a pure function of (seed, start + i) --
 * a pose near a lemniscate course, its speed and previous controls, and a plan of M waypoints
 * along the course -- so a rank of a multi-GPU run generates exactly its own slice on its GPU.
 * Outputs as mpcg_preprocess_device takes them: pose [B][3], vel [B][3], plan [B][M][2].  Not
 * part of the reference's interface (a data generator for benchmarks and tests); queued on
 * `stream` (the first call uploads a 3.2 MB table synchronously). */
int mpcg_synth_infinity_device(mpcg_handle* h, uint64_t seed, int64_t start, int64_t B, int32_t M, double* d_pose,
                               double* d_vel, double* d_plan, void* stream);

/* Kernel strategy of the handle's solves.  Since ABI 2 there is one: one problem per
 * wavefront, the whole problem state in LDS (AUTO and WAVE select it).  LANE (the round-1
 * one-problem-per-lane kernels) was removed; selecting it is an error. */
#define MPCG_STRATEGY_AUTO 0
#define MPCG_STRATEGY_LANE 1
#define MPCG_STRATEGY_WAVE 2
int mpcg_set_strategy(mpcg_handle* h, int32_t strategy);
/* The strategy a solve of the handle's current parameters would use (never AUTO). */
int mpcg_get_strategy(const mpcg_handle* h);

/* Wait for all work queued on the handle's stream. */
int mpcg_synchronize(mpcg_handle* h);

#ifdef __cplusplus
}
#endif
#endif
