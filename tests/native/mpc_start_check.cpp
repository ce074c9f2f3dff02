// tests/native/mpc_start_check.cpp -- the drop-in class MPC's extension start_from_solution /
// last_start_used() (include/mpc_planner.h), beside mpc_solution_check.cpp.
//
// stdin: lines of state[6] coeffs[4], a chain of neighbouring problems.
// stdout: per line "cold <iters> <w0> <a0>" (a default MPC's Solve of the line), then per line
//         "start <used> <iters> <w0> <a0>" (one MPC with start_from_solution(MPCG_START_FULL)
//         solving the chain in order), every double as %.17g
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "mpc_planner.h"

int main() {
    std::map<std::string, double> p;  // MPCPlanner.cfg defaults, DT = 0.1
    p["DT"] = 0.1; p["STEPS"] = 20; p["REF_CTE"] = 0.0; p["REF_ETHETA"] = 0.0; p["REF_V"] = 1.0;
    p["W_CTE"] = 1000; p["W_EPSI"] = 1000; p["W_V"] = 100; p["W_ANGVEL"] = 100; p["W_A"] = 50;
    p["W_DANGVEL"] = 0; p["W_DA"] = 10; p["ANGVEL"] = 1.0; p["MAXTHR"] = 1.0; p["BOUND"] = 1000;
    std::vector<std::vector<double>> lines;
    for (;;) {
        std::vector<double> v(10);
        bool ok = true;
        for (double& x : v)
            if (std::scanf("%lf", &x) != 1) ok = false;
        if (!ok) break;
        lines.push_back(v);
    }
    MPC cold;
    cold.LoadParams(p);
    for (const auto& v : lines) {
        std::vector<double> state(v.begin(), v.begin() + 6), coeffs(v.begin() + 6, v.end());
        std::vector<double> r = cold.Solve(state, coeffs);
        if (cold.last_start_used() != MPCG_START_COLD) return 2;
        std::printf("cold %d %.17g %.17g\n", cold.last_iters(), r[0], r[1]);
    }
    MPC mpc;
    mpc.LoadParams(p);
    mpc.start_from_solution(MPCG_START_FULL);
    for (const auto& v : lines) {
        std::vector<double> state(v.begin(), v.begin() + 6), coeffs(v.begin() + 6, v.end());
        std::vector<double> r = mpc.Solve(state, coeffs);
        std::printf("start %d %d %.17g %.17g\n", mpc.last_start_used(), mpc.last_iters(), r[0], r[1]);
    }
    return 0;
}
