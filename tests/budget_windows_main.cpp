// The program tests/test_budget_windows_host.py builds (g++, address and undefined-behaviour sanitizers) and runs:
// csrc/budget_root.h and csrc/budget_win_map.h alone, no HIP.
// stdin, one request per line:
//   map rows n_win a0 win_end[0..n_win)
//        -> "map units=<rows * n_win> g j t0 t1 ..." : budget_win_unit of every unit u = 0 .. rows * n_win - 1, as the kernel's waves
//           take them
//   row T n_win max_evals win_end[0..n_win) e_min[0..n_win) e_max[0..n_win) then per step: cap m(kinks) xk[max(m,1)] vk[max(m,1)] sl[m + 1]
//        (hexadecimal doubles; inf allowed)
//        -> "row fails=<units out of evaluations> nu[0] .. nu[n_win-1] x[0] .. x[T-1]" (hexadecimal doubles): k_gen_budget_win's phase 1 for
//           one row — every unit of the row runs budget_root over its own window and stores x(nu*) there (a unit out of evaluations:
//           nu = 0, the clamped step)
// A step is the increasing piecewise-linear derivative phi_t of the step's objective, as tests/helpers_ramp_net.py writes it:
// x_t(nu) = clip(phi_t^{-1}(-nu), 0, cap_t).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "budget_root.h"
#include "budget_win_map.h"

using namespace dopf;

struct HostStep {
    double cap;
    std::vector<double> xk, vk, sl;
    double at(double nu, int &piece) const
    {
        const int m = (int)sl.size() - 1;
        const double want = -nu;
        int j = 0;
        while (j < m && vk[(size_t)j] < want) ++j;
        const int a = j < m ? j : (m > 0 ? m - 1 : 0);
        const double u = xk[(size_t)a] + (want - vk[(size_t)a]) / sl[(size_t)j];
        piece = budget_piece(u, cap, j);
        return u < 0.0 ? 0.0 : (u > cap ? cap : u);
    }
};

static bool read_doubles(std::vector<double> &a, int n)
{
    a.resize((size_t)n);
    for (double &x : a) if (scanf("%la", &x) != 1) return false;
    return true;
}

static bool read_ints(std::vector<int> &a, int n)
{
    a.resize((size_t)n);
    for (int &x : a) if (scanf("%d", &x) != 1) return false;
    return true;
}

int main()
{
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "map")) {
            int rows, n_win, a0;
            std::vector<int> end;
            if (scanf("%d %d %d", &rows, &n_win, &a0) != 3 || rows < 0 || n_win < 1 || !read_ints(end, n_win)) return 2;
            const int units = rows * n_win;
            printf("map units=%d", units);
            for (int u = 0; u < units; ++u) {
                const BudgetUnit un = budget_win_unit(u, a0, n_win, end.data());
                printf(" %d %d %d %d", un.g, un.j, un.t0, un.t1);
            }
            printf("\n");
        } else if (!strcmp(what, "row")) {
            int T, n_win, max_evals;
            std::vector<int> end;
            std::vector<double> e_min, e_max;
            if (scanf("%d %d %d", &T, &n_win, &max_evals) != 3 || T < 1 || n_win < 1 || !read_ints(end, n_win) || !read_doubles(e_min, n_win) ||
                !read_doubles(e_max, n_win) || end[(size_t)n_win - 1] != T)
                return 2;
            std::vector<HostStep> row((size_t)T);
            for (HostStep &s : row) {
                int m;
                if (scanf("%la %d", &s.cap, &m) != 2 || m < 0) return 2;
                const int n = m > 0 ? m : 1;
                if (!read_doubles(s.xk, n) || !read_doubles(s.vk, n) || !read_doubles(s.sl, m + 1)) return 2;
            }
            std::vector<double> x((size_t)T), nus((size_t)n_win);
            int fails = 0;
            for (int u = 0; u < n_win; ++u) {           // the row's units, a0 = 0: unit u is (row 0, window u)
                const BudgetUnit un = budget_win_unit(u, 0, n_win, end.data());
                if (un.g != 0 || un.j != u || un.t0 < 0 || un.t1 > T || un.t0 >= un.t1) return 3;
                double steepest = 0.0;
                for (int t = un.t0; t < un.t1; ++t)
                    for (double v : row[(size_t)t].sl) steepest = std::fmax(steepest, 1.0 / v);
                auto probe = [&](double a, double m, double b) {
                    double sum = 0.0;
                    BudgetSame sm;
                    for (int t = un.t0; t < un.t1; ++t) {
                        int pa, pm, pb;
                        row[(size_t)t].at(a, pa);
                        sum += row[(size_t)t].at(m, pm);
                        row[(size_t)t].at(b, pb);
                        sm.add(pa, pm, pb);
                    }
                    return BudgetProbe{sum, sm.sameA, sm.sameB, sm.atLo, sm.atHi};
                };
                double phi0 = 0.0;
                int piece;
                for (int t = un.t0; t < un.t1; ++t) phi0 += row[(size_t)t].at(0.0, piece);
                const double lo = e_min[(size_t)u], hi = e_max[(size_t)u];
                const double off = phi0 > hi ? phi0 - hi : lo - phi0;
                double nu = 0.0;
                int evals = 0;
                const int rc = budget_root(probe, phi0, lo, hi, std::fmax(off / ((double)(un.t1 - un.t0) * steepest), 1e-12), max_evals, &nu, &evals);
                if (rc < 0) { nu = 0.0; ++fails; }
                nus[(size_t)u] = nu;
                for (int t = un.t0; t < un.t1; ++t) x[(size_t)t] = row[(size_t)t].at(nu, piece);
            }
            printf("row fails=%d", fails);
            for (double v : nus) printf(" %a", v);
            for (double v : x) printf(" %a", v);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
