// tests/native/mpc_gain_check.cpp -- the drop-in class MPC (include/mpc_planner.h) with
// keep_solution(true): the feedback gain of every Solve beside the record it was computed from.
//
// stdin: lines of state[6] coeffs[4]; stdout per line: w0 a0, gain_info, the 20 entries of
// feedback_gain(), then the record solution().  Before the first Solve the gain is empty and the
// flag -1 (exit code 3 otherwise).
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "mpc_planner.h"

int main() {
    std::map<std::string, double> mpc_params;  // MPCPlanner.cfg defaults, DT = 0.1
    mpc_params["DT"] = 0.1;
    mpc_params["STEPS"] = 20;
    mpc_params["REF_CTE"] = 0.0;
    mpc_params["REF_ETHETA"] = 0.0;
    mpc_params["REF_V"] = 1.0;
    mpc_params["W_CTE"] = 1000;
    mpc_params["W_EPSI"] = 1000;
    mpc_params["W_V"] = 100;
    mpc_params["W_ANGVEL"] = 100;
    mpc_params["W_A"] = 50;
    mpc_params["W_DANGVEL"] = 0;
    mpc_params["W_DA"] = 10;
    mpc_params["ANGVEL"] = 1.0;
    mpc_params["MAXTHR"] = 1.0;
    mpc_params["BOUND"] = 1000;
    MPC mpc;
    mpc.LoadParams(mpc_params);
    mpc.keep_solution(true);
    if (!mpc.feedback_gain().empty() || mpc.gain_info() != -1) return 3;
    std::vector<double> state(6), coeffs(4);
    while (true) {
        for (double& v : state)
            if (std::scanf("%lf", &v) != 1) return 0;
        for (double& v : coeffs)
            if (std::scanf("%lf", &v) != 1) return 1;
        std::vector<double> r = mpc.Solve(state, coeffs);
        std::printf("%.17g %.17g %d", r[0], r[1], mpc.gain_info());
        for (double g : mpc.feedback_gain()) std::printf(" %.17g", g);
        for (double x : mpc.solution()) std::printf(" %.17g", x);
        std::printf("\n");
        std::fflush(stdout);
    }
}
