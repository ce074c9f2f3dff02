/*
 * include/mpc_planner.h -- drop-in replacement of the reference's
 * mpc_ros/include/mpc_planner.h (class MPC, :26-47), backed by libmpcg.so.
 *
 * The move_base plugin (mpc_ros/src/mpc_planner_ros.cpp) and the driving-state
 * FSM (mpc_ros/src/driving_state.cpp:260) compile against this header unchanged:
 *   MPC();  void LoadParams(const std::map<string,double>&);
 *   vector<double> Solve(Eigen::VectorXd state, Eigen::VectorXd coeffs);  -> {w0, a0}
 *   vector<double> mpc_x, mpc_y, mpc_theta;
 * Solve is a template over the vector type so that Eigen::VectorXd (when the caller
 * has Eigen) and std::vector<double> both work; arguments are taken by value, as in
 * the reference.  Extensions: SolveBatch (B robots per call) and the last solve's
 * status / iteration count / objective.
 */
#ifndef MPCG_MPC_PLANNER_H
#define MPCG_MPC_PLANNER_H

#include <map>
#include <string>
#include <vector>

#include "mpcg.h"

using namespace std;  // the reference header does this (mpc_planner.h:24); kept for source compatibility

class MPC {
   public:
    MPC();
    ~MPC();
    MPC(const MPC& o);             // DrivingStateContext::getMpc() copies (driving_state.h:79)
    MPC& operator=(const MPC& o);

    // Solve the model given an initial state and polynomial coefficients.
    // Return the first actuations {angular velocity, acceleration}.
    template <class Vec>
    vector<double> Solve(Vec state, Vec coeffs) {
        double s[6], c[4];
        for (int i = 0; i < 6; ++i) s[i] = static_cast<double>(state[i]);
        for (int i = 0; i < 4; ++i) c[i] = static_cast<double>(coeffs[i]);
        return SolveRaw(s, c);
    }
    vector<double> mpc_x;
    vector<double> mpc_y;
    vector<double> mpc_theta;

    void LoadParams(const std::map<string, double>& params);

    // ---- extensions (not in the reference) ----
    // B problems in one GPU launch; state [B][6], coeffs [B][4], u0 [B][2],
    // traj [B][3][N] (or null), status [B] (or null).  Returns 0 or a negative mpcg code.
    int SolveBatch(int64_t B, const double* state, const double* coeffs, double* u0, double* traj,
                   int32_t* status);
    int last_status() const { return _last_status; }
    int last_iters() const { return _last_iters; }
    double last_obj() const { return _last_obj; }
    int steps() const { return _mpc_steps; }
    // The full solution of the last Solve (include/mpcg.h mpcg_solve_sol): x | zl | zu | lambda of
    // the unscaled NLP, mpcg_solution_elems(steps()) doubles.  Off by default -- a default Solve
    // copies nothing more; empty until a Solve has run with it on.
    void keep_solution(bool on) { _keep_solution = on; }
    const vector<double>& solution() const { return _solution; }
    // The feedback law around the last Solve's solution (include/mpcg.h mpcg_sens, evaluated on the
    // host from the kept record): 2 x 10 doubles, row-major, d(w0, a0) / d(state[0..5], coeffs[0..3]);
    // u = clip(u0 + gain [dstate; dcoeffs]) corrects the command for a measured state that differs
    // from the predicted one without another Solve.  Needs keep_solution(true); empty before such a
    // Solve.  gain_info(): mpcg_sens's flag (0 valid; 1, 2: the gain is NaN), -1 before such a Solve.
    const vector<double>& feedback_gain() const { return _gain; }
    int gain_info() const { return _gain_info; }
    // Start point in (include/mpcg.h mpcg_solve_start): with a mode other than MPCG_START_COLD a
    // Solve keeps its solution record and the next Solve starts from it as it is -- in the vehicle
    // frame consecutive ticks solve almost the same problem, and the unshifted record is the
    // natural start.  MPCG_START_PRIMAL takes the record's x; MPCG_START_FULL takes x and the
    // multipliers, with the barrier parameter mu0 (the final mu of a converged solve, ~1e-9, leaves
    // the line search no room; 1e-4 is a default in the range Ipopt users set mu_init to for warm
    // starts, not a tuned value).  The default mode is MPCG_START_COLD: a default Solve is unchanged
    // and copies nothing more.  A Solve runs cold while there is no record or STEPS has changed, and
    // after a Solve whose status is neither 1 (success) nor 4 (acceptable point).
    // last_start_used(): the mode the last Solve ran in (mpcg_solve_start's start_used).
    void start_from_solution(int mode, double mu0 = 1e-4) {
        _start_mode = mode;
        _start_mu0 = mu0;
        if (mode == MPCG_START_COLD) _start_rec.clear();
    }
    int last_start_used() const { return _start_used; }
    // The robot's motion since the last Solve, for the next Solve with start_from_solution on: the
    // new vehicle frame's origin (dx, dy) and heading dpsi expressed in the last Solve's frame.  The
    // kept record is shifted by one stage and moved to the new frame (include/mpcg.h
    // mpcg_shift_solution; a control period equal to DT) before it is used.  One-shot: it applies to
    // the next Solve only; without it that Solve starts from the record as it is.
    void carry_motion(double dx, double dy, double dpsi) {
        _carry[0] = dx;
        _carry[1] = dy;
        _carry[2] = dpsi;
        _have_carry = true;
    }
    // GPU the solver runs on (default 0); call before the first Solve.
    void set_device(int device) { _device = device; }

   private:
    vector<double> SolveRaw(const double* state, const double* coeffs);
    int ensure_handle();
    mpcg_params effective_params() const;

    // Parameters for mpc solver (same members as the reference, mpc_planner.h:40-43)
    double _max_angvel, _max_throttle, _bound_value;
    int _mpc_steps, _x_start, _y_start, _theta_start, _v_start, _cte_start, _etheta_start, _angvel_start, _a_start;
    std::map<string, double> _params;

    int _device;
    mpcg_handle* _handle;
    int _last_status, _last_iters;
    double _last_obj;
    bool _keep_solution = false;
    vector<double> _solution;
    vector<double> _gain;
    int _gain_info = -1;
    int _start_mode = MPCG_START_COLD, _start_used = MPCG_START_COLD;
    double _start_mu0 = 1e-4;
    vector<double> _start_rec;  // the last Solve's record while start_from_solution is on
    double _carry[3] = {0, 0, 0};  // carry_motion's argument while _have_carry
    bool _have_carry = false;
};

#endif /* MPCG_MPC_PLANNER_H */
