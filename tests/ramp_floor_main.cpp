// The program tests/test_ramp_floor_host.py builds (g++, address and undefined-behaviour sanitizers) and runs: csrc/ramp_dp.h alone,
// no HIP — ramp_repair_pwl<true>, the routine a lane of k_gen_ramp_net<.., .., true> runs on a row with a floor.
// stdin, one request per line:
//   row T K up down prev(NaN: none) then per step: floor cap m(kinks) xk[max(m,1)] vk[max(m,1)] sl[m + 1]   (hexadecimal doubles)
//                                   -> "row ok=<0|1> guard=<0|1> x[0] .. x[T-1]" (hexadecimal doubles; with ok=0 the row's T
//                                      start values, untouched). The knots live in heap arrays of exactly K doubles: a write
//                                      beyond the capacity is the address sanitizer's to report. guard: the output row is as it was.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ramp_dp.h"

using namespace dopf;

struct HostRow {
    std::vector<double> caps, floors;
    std::vector<std::vector<double>> xk, vk, sl;
    double cap(int t) const { return caps[(size_t)t]; }
    double floor(int t) const { return floors[(size_t)t]; }
    RampStepPwl step(int t) const
    {
        return RampStepPwl{(int)sl[(size_t)t].size() - 1, xk[(size_t)t].data(), vk[(size_t)t].data(), sl[(size_t)t].data()};
    }
};

static bool read_doubles(std::vector<double> &a, int n)
{
    a.resize((size_t)n);
    for (double &x : a) if (scanf("%la", &x) != 1) return false;
    return true;
}

int main()
{
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "row")) {
            int T, K;
            double up, down, prev;
            if (scanf("%d %d %la %la %la", &T, &K, &up, &down, &prev) != 5 || T < 1 || K < 0) return 2;
            HostRow row;
            row.caps.resize((size_t)T); row.floors.resize((size_t)T); row.xk.resize((size_t)T); row.vk.resize((size_t)T); row.sl.resize((size_t)T);
            for (int t = 0; t < T; ++t) {
                int m;
                if (scanf("%la %la %d", &row.floors[(size_t)t], &row.caps[(size_t)t], &m) != 3 || m < 0) return 2;
                const int n = m > 0 ? m : 1;
                if (!read_doubles(row.xk[(size_t)t], n) || !read_doubles(row.vk[(size_t)t], n) || !read_doubles(row.sl[(size_t)t], m + 1)) return 2;
            }
            // exactly K doubles each, on the heap: the sanitizer's red zones stand right behind them
            double *kx = new double[(size_t)K], *kv = new double[(size_t)K], *cy = new double[(size_t)T];
            std::vector<double> out((size_t)T);
            for (int t = 0; t < T; ++t) out[(size_t)t] = -1.0 - t;
            const std::vector<double> was(out);
            const bool ok = ramp_repair_pwl<true>(row, out.data(), cy, kx, kv, K, T, up, down, prev);
            printf("row ok=%d guard=%d", ok ? 1 : 0, out == was ? 1 : 0);
            for (int t = 0; t < T; ++t) printf(" %a", out[(size_t)t]);
            printf("\n");
            delete[] kx; delete[] kv; delete[] cy;
        } else {
            return 2;
        }
    }
    return 0;
}
