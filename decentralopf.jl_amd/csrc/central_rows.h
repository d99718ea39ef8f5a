// central_rows.h — the per-row arithmetic of the coupled device LP (dopf_central_solve_coupled): a generator column's
// primal step under ramp and budget rows, the rows' proximal steps, their terms of the dual objective and their violations.
// Plain C++, no HIP include: kc_gen_rows (kernels_central.hip) runs it on the lanes of the wave that owns a generator row,
// tests/central_rows_main.cpp as a host program under sanitizers.
//
//   ramp rows     t >= 1:        -rd <= P[t] - P[t-1] <= ru            multiplier yR[t]
//                 t = 0, anchor: prev - rd <= P[0] <= prev + ru        multiplier yR[0]   (no anchor: no row, yR[0] = 0)
//   budget row    e_min <= sum_t P[t] <= e_max                         multiplier yQ
//   a multiplier is positive where the row's upper end binds, negative where the lower one does (the flow rows' convention)
//   column (g,t)  reduced cost mc + pi + yR[t] - yR[t+1] + yQ, step 1 / ((1 + absH + a + b) w) with a = the ramp rows that touch the
//                 column and b = 1 with a budget row (Pock & Chambolle: the column's sum of |K|)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_CR_FN __host__ __device__ inline
#else
#define DOPF_CR_FN inline
#endif

namespace dopf {

constexpr double kCrInf = __builtin_huge_val();

DOPF_CR_FN double cr_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// which rows a generator has: ramp rows with a finite limit or an anchor (NaN: none), a budget row with e_min > 0 or a finite e_max
DOPF_CR_FN bool cr_anchored(double prev) { return prev == prev; }
DOPF_CR_FN bool cr_has_ramp(double ru, double rd, double prev) { return ru < kCrInf || rd < kCrInf || cr_anchored(prev); }
DOPF_CR_FN bool cr_has_budget(double e_min, double e_max) { return e_min > 0.0 || e_max < kCrInf; }

// a: the generator's ramp rows that touch column t — its own row (t >= 1, or t = 0 with an anchor) and the row of t + 1
DOPF_CR_FN int cr_ramp_rows_at(int t, int T, bool ramp, bool anchored)
{
    if (!ramp) return 0;
    return ((t >= 1 || anchored) ? 1 : 0) + (t + 1 < T ? 1 : 0);
}

DOPF_CR_FN double cr_tau(double absH, int a, int b, double w) { return 1.0 / ((1.0 + absH + (double)(a + b)) * w); }

// the bounds of ramp row t: the difference's at t >= 1, the anchor's at t = 0
DOPF_CR_FN double cr_ramp_lo(int t, double rd, double prev) { return t >= 1 ? -rd : prev - rd; }
DOPF_CR_FN double cr_ramp_hi(int t, double ru, double prev) { return t >= 1 ? ru : prev + ru; }
// row sums of |K|: a difference has two entries, the anchor's row one, the budget row T
DOPF_CR_FN double cr_sigma_ramp(int t, double w) { return t >= 1 ? w / 2.0 : w; }
DOPF_CR_FN double cr_sigma_budget(int T, double w) { return w / (double)T; }

// (absent rows: multipliers of 0)
DOPF_CR_FN double cr_reduced_cost(double mc, double pi, double yR, double yR_next, double yQ) { return mc + pi + yR - yR_next + yQ; }

DOPF_CR_FN double cr_column_step(double x0, double tau, double rc, double cap) { return cr_clamp(x0 - tau * rc, 0.0, cap); }

// y+ = z - sigma clamp(z / sigma, lo, hi) with z = y + sigma row(2x+ - x): the proximal step of the interval's support function, as
// the flow rows take it — written by cases, so that a row whose value lies inside its interval gets a multiplier of exactly 0: what
// z - sigma (z / sigma) leaves is a rounding error of either sign, and on the side of an infinite end the dual objective would
// multiply it by that end
DOPF_CR_FN double cr_prox(double y, double sigma, double row, double lo, double hi)
{
    const double z = y + sigma * row, q = z / sigma;
    if (q < lo) return z - sigma * lo;
    if (q > hi) return z - sigma * hi;
    return 0.0;
}

// the row's term of the dual objective, -(max(y, 0) hi + min(y, 0) lo), by selects: 0 * inf is NaN and a one-sided row has an infinite end
DOPF_CR_FN double cr_support(double y, double lo, double hi)
{
    const double up = y > 0.0 ? y * hi : 0.0, dn = y < 0.0 ? y * lo : 0.0;
    return -(up + dn);
}

// the column's term of the dual objective: min over the box [0, cap] of rc x
DOPF_CR_FN double cr_rc_term(double rc, double cap) { return (rc < 0.0 ? rc : 0.0) * cap; }

// how far the row's value lies outside [lo, hi] (0 inside)
DOPF_CR_FN double cr_violation(double row, double lo, double hi)
{
    const double a = lo - row, b = row - hi, m = a > b ? a : b;
    return m > 0.0 ? m : 0.0;
}

}  // namespace dopf
