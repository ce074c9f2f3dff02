// tests/native/mpc_carry_check.cpp -- the drop-in class MPC's extension carry_motion
// (include/mpc_planner.h), beside mpc_start_check.cpp.
//
// stdin: lines of state[6] coeffs[4] motion[3] flag, a chain of consecutive problems; flag 1: the
//        line's motion is given to carry_motion before its Solve, 0: it is not.
// stdout: per line "carry <used> <iters> <w0> <a0>" -- one MPC with
//         start_from_solution(MPCG_START_PRIMAL) solving the chain in order -- then the record the
//         last Solve kept, "sol <n> <values>", every double as %.17g
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
        std::vector<double> v(14);
        bool ok = true;
        for (double& x : v)
            if (std::scanf("%lf", &x) != 1) ok = false;
        if (!ok) break;
        lines.push_back(v);
    }
    MPC mpc;
    mpc.LoadParams(p);
    mpc.keep_solution(true);
    mpc.start_from_solution(MPCG_START_PRIMAL);
    for (const auto& v : lines) {
        std::vector<double> state(v.begin(), v.begin() + 6), coeffs(v.begin() + 6, v.begin() + 10);
        if (v[13] != 0.0) mpc.carry_motion(v[10], v[11], v[12]);
        std::vector<double> r = mpc.Solve(state, coeffs);
        std::printf("carry %d %d %.17g %.17g\n", mpc.last_start_used(), mpc.last_iters(), r[0], r[1]);
    }
    std::printf("sol %zu", mpc.solution().size());
    for (double x : mpc.solution()) std::printf(" %.17g", x);
    std::printf("\n");
    return 0;
}
