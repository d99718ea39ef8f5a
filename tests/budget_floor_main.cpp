// The program tests/test_budget_floor_host.py builds (g++, address and undefined-behaviour sanitizers) and runs: csrc/budget_root.h
// alone, no HIP. It is tests/budget_main.cpp's root request with a floor per step (dopf_set_generator_budget_min_output):
// the pieces come from the four-argument budget_piece, the clip is [floor_t, cap_t].
// stdin, one request per line:
//   root T e_min e_max max_evals then per step: floor cap m(kinks) xk[max(m,1)] vk[max(m,1)] sl[m + 1]   (hexadecimal doubles; inf allowed)
//        -> "root rc=<budget_root's> evals=<n> nu=<hex> x[0] .. x[T-1]" (hexadecimal doubles): the row's step at the multiplier found
//           (rc = -1: at 0, the clamped step, as the kernel keeps it)
// A step is the increasing piecewise-linear derivative phi_t of the step's objective, as tests/helpers_ramp_net.py writes it:
// x_t(nu) = clip(phi_t^{-1}(-nu), floor_t, cap_t).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "budget_root.h"

using namespace dopf;

struct HostStep {
    double floor, cap;
    std::vector<double> xk, vk, sl;
    // x_t(nu) and its linear piece
    double at(double nu, int &piece) const
    {
        const int m = (int)sl.size() - 1;
        const double want = -nu;
        int j = 0;
        while (j < m && vk[(size_t)j] < want) ++j;
        const int a = j < m ? j : (m > 0 ? m - 1 : 0);
        const double u = xk[(size_t)a] + (want - vk[(size_t)a]) / sl[(size_t)j];
        piece = budget_piece(u, floor, cap, j);
        return u < floor ? floor : (u > cap ? cap : u);
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
        if (strcmp(what, "root")) return 2;
        int T, max_evals;
        double e_min, e_max;
        if (scanf("%d %la %la %d", &T, &e_min, &e_max, &max_evals) != 4 || T < 1) return 2;
        std::vector<HostStep> row((size_t)T);
        double steepest = 0.0;
        for (HostStep &s : row) {
            int m;
            if (scanf("%la %la %d", &s.floor, &s.cap, &m) != 3 || m < 0 || !(s.floor >= 0.0 && s.floor <= s.cap)) return 2;
            const int n = m > 0 ? m : 1;
            if (!read_doubles(s.xk, n) || !read_doubles(s.vk, n) || !read_doubles(s.sl, m + 1)) return 2;
            for (double v : s.sl) steepest = std::fmax(steepest, 1.0 / v);
        }
        auto sum_at = [&](double nu) {
            double sum = 0.0;
            int piece;
            for (const HostStep &s : row) sum += s.at(nu, piece);
            return sum;
        };
        auto probe = [&](double a, double m, double b) {
            double sum = 0.0;
            BudgetSame sm;
            for (const HostStep &s : row) {
                int pa, pm, pb;
                s.at(a, pa);
                sum += s.at(m, pm);
                s.at(b, pb);
                sm.add(pa, pm, pb);
            }
            return BudgetProbe{sum, sm.sameA, sm.sameB, sm.atLo, sm.atHi};
        };
        const double phi0 = sum_at(0.0);
        const double off = phi0 > e_max ? phi0 - e_max : e_min - phi0;
        double nu = 0.0;
        int evals = 0;
        const int rc = budget_root(probe, phi0, e_min, e_max, std::fmax(off / (T * steepest), 1e-12), max_evals, &nu, &evals);
        if (rc < 0) nu = 0.0;
        printf("root rc=%d evals=%d nu=%a", rc, evals, nu);
        for (const HostStep &s : row) { int piece; printf(" %a", s.at(nu, piece)); }
        printf("\n");
    }
    return 0;
}
