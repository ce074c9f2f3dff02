// tests/native/window_check.cpp -- mpc_ros_amd/csrc/mpcg_window.h (the plan window the kernel
// k_plan_window and mpcg_plan_window run) on the host, for AddressSanitizer + UBSan
// (tests/test_plan_window.py): courses and plans in heap buffers of exactly their size, so a
// read past the course or a write past the Mmax rows is reported.  Checks the rule's invariants
// on every case and prints the number of cases.
//   g++ -std=c++17 -fsanitize=address,undefined -I mpc_ros_amd/csrc -I include -o window_check window_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mpcg_window.h"

static unsigned long long rng_state = 20251015ULL;
static double uniform() {  // splitmix64 -> [0, 1)
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);    \
            return 1;                                              \
        }                                                          \
    } while (0)

int main() {
    const int Gs[] = {1, 2, 5, 37, 400};
    const int wps[] = {1, 3, 4, 10, 31, 100, 1000, 2147483647};
    const int strides[] = {1, 3, 10, 64, 2147483647};
    long cases = 0;
    for (int G : Gs) {
        std::vector<double> course(2 * (size_t)G);
        for (int i = 0; i < G; ++i) {
            course[2 * i] = 0.05 * i + 0.01 * uniform();
            course[2 * i + 1] = 0.002 * i * i * 0.05;
        }
        for (int wp : wps)
            for (int stride : strides) {
                const int64_t mmax64 = mpcg::plan_window_mmax(wp, stride);
                CHECK(mmax64 >= 2);
                // the rows a window of this course can fill (the device call refuses Mmax > 64;
                // the host function takes any, so the buffer here is what the course can need)
                const int rows = (int)(mmax64 < (int64_t)G + 1 ? mmax64 : (int64_t)G + 1);
                for (int rep = 0; rep < 40; ++rep) {
                    const int c = (int)(uniform() * G);
                    const int k = (int)(uniform() * G);
                    const double x = rep == 0 ? 2000.0 : course[2 * k] + 0.04 * (uniform() - 0.5);
                    const double y = course[2 * k + 1] + 0.04 * (uniform() - 0.5);
                    const mpcg::PlanWindow w = mpcg::plan_window(course.data(), G, c, x, y, wp, stride);
                    CHECK(w.start >= c && w.start <= G);
                    CHECK(w.cursor >= c && w.cursor < G && (w.cursor == c || w.cursor == w.start - 1));
                    CHECK(w.W >= 0 && w.W <= wp && w.start + w.W <= G);
                    CHECK(w.count == (w.W ? (w.W + (int64_t)stride - 1) / stride + 1 : 0));
                    CHECK(w.count <= rows);
                    if (rep == 0) CHECK(w.start == c);  // (beyond 1000 m: nothing erased)
                    for (int j = 0; j < w.count; ++j) {
                        const int g = mpcg::plan_window_index(w, stride, j);
                        CHECK(g >= w.start && g < w.start + w.W);
                        CHECK(j == 0 || g >= mpcg::plan_window_index(w, stride, j - 1));
                    }
                    std::vector<double> plan(2 * (size_t)rows, 7.0);
                    mpcg::plan_window_copy(course.data(), w, stride, rows, plan.data());
                    for (int j = 0; j < rows; ++j) {
                        const int g = j < w.count ? mpcg::plan_window_index(w, stride, j) : -1;
                        CHECK(plan[2 * j] == (g < 0 ? 0.0 : course[2 * g]));
                        CHECK(plan[2 * j + 1] == (g < 0 ? 0.0 : course[2 * g + 1]));
                    }
                    ++cases;
                }
            }
    }
    std::printf("window_check: %ld cases ok\n", cases);
    return 0;
}
