// budget_win_map.h — energy budgets per sub-window (dopf_set_generator_energy_budget_windows): what the kernel is handed
// and how an item's work is cut into units. Plain C++, no HIP include: gen_budget_win.h runs it on the device,
// tests/budget_windows_main.cpp as a host program under sanitizers.
//
// Window j of n_win covers the timesteps win_end[j-1] <= t < win_end[j] (win_end[-1] = 0, win_end[n_win-1] = T). The windows are
// disjoint, so a row under n_win budgets is n_win rows of budget_root.h's kind, one multiplier each: a unit is a (row, window) pair.
#pragma once

#include "budget_root.h"

namespace dopf {

// the kernel's second argument, by value next to DevView (which keeps its size): device arrays of the context's own, rows in sorted
// order, [j + n_win * g]. n_win == 0: no table (Plan::genBudgetWin of a context that runs k_gen_budget)
struct BudgetWinView {
    const int *end;                 // n_win
    const double *emin, *emax;      // n_win x G
    double *nu;                     // n_win x G: the multiplier the last x-update put on each window's row
    int n_win;
};

struct BudgetUnit {
    int g, j, t0, t1;               // the row, its window and the window's timesteps t0 <= t < t1
};

// unit u of an item whose rows begin at a0: rows outermost, so that with n_win = 1 unit u is row a0 + u over [0, T)
DOPF_BR_FN BudgetUnit budget_win_unit(int u, int a0, int n_win, const int *win_end)
{
    const int r = u / n_win, j = u - r * n_win;
    return BudgetUnit{a0 + r, j, j > 0 ? win_end[j - 1] : 0, win_end[j]};
}

}  // namespace dopf
