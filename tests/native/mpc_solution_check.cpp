// tests/native/mpc_solution_check.cpp -- the drop-in class MPC's extension keep_solution /
// solution() (include/mpc_planner.h), beside mpc_class_check.cpp's reference members.
//
// stdin: lines of state[6] coeffs[4]; the first line is solved as a default MPC solves it (nothing
// kept), every line then with keep_solution(true).
// stdout: first "kept <n>" (the record's size after the default Solve: 0), then per line
//         w0 a0 and the record, every double as %.17g
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
    MPC mpc;
    mpc.LoadParams(p);
    std::vector<double> state(6), coeffs(4);
    for (bool first = true;; first = false) {
        for (double& v : state)
            if (std::scanf("%lf", &v) != 1) return 0;
        for (double& v : coeffs)
            if (std::scanf("%lf", &v) != 1) return 1;
        if (first) {
            mpc.Solve(state, coeffs);
            std::printf("kept %zu\n", mpc.solution().size());
            mpc.keep_solution(true);
        }
        std::vector<double> r = mpc.Solve(state, coeffs);
        std::printf("%.17g %.17g", r[0], r[1]);
        for (double x : mpc.solution()) std::printf(" %.17g", x);
        std::printf("\n");
        std::fflush(stdout);
    }
}
