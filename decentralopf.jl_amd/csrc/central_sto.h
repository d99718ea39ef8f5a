// central_sto.h — the per-timestep arithmetic of the device LP's storage (level) rows (kc_sto, kc_sto_long in kernels_central.hip;
// DESIGN.md 5n): a storage's two columns' primal steps, the level row's proximal step, its term of the dual objective and its violation.
// Plain C++, no HIP include: both kernels run these functions on whatever thread owns a timestep — they differ in who that is, how a
// neighbour's sum arrives and how the item's sums are kept, not in a statement below — and tests/central_sto_main.cpp runs them as a
// host program under sanitizers.
//
//   level row t    lb_t - e0 <= sum_{tau <= t} (be C - al D) <= ub_t - e0        multiplier yE[t], positive where the upper end binds
//                  [lb_t, ub_t] = [0, em], at t = T-1 with LV >= 2 [elo, ehi]
//   LV             Plan::stoLV. 0: e0 = 0, no band, al = be = 1; 1: e0; 2: e0 and the band; 3: e0, the band, al = 1 / eta_d, be = eta_c.
//                  A lower LV's statements are kept as they are (not LV 3's with ones and zeros put in): each has its own roundings and its
//                  own fusions on the device, and tests/test_central_sto_host.py pins what the levels share.
//   columns (s,t)  rD = mc + pi - al suf, rC = mc - pi + be suf with suf = sum_{tau >= t} yE; steps 1 / ((1 + absH + al (T - t)) w),
//                  ... be (T - t) (Pock & Chambolle: the column's sum of |K|), one step for both below LV 3
//
// cs_clamp and cs_prox are NOT central_rows.h's cr_clamp and cr_prox: these clamp with fmin / fmax and subtract sigma clamp(z / sigma)
// whatever the case (the flow rows' step, kc_dual), those select by comparisons and return an exact 0 inside the interval, for rows
// with an infinite end. Different operations, different bits — the two stay apart.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_CS_FN __host__ __device__ inline
#else
#define DOPF_CS_FN inline
#endif

namespace dopf {

// one storage's constants (below LV 1: e0 = 0; below LV 2: [elo, ehi] = [0, em]; below LV 3: al = be = 1 — set, and never read)
struct StoRow {
    double mc, pm, em, e0, elo, ehi, al, be;
};

DOPF_CS_FN double cs_clamp(double v, double lo, double hi) { return __builtin_fmin(__builtin_fmax(v, lo), hi); }

// the extrapolated point 2x+ - x of one column
DOPF_CS_FN double cs_extra(double xn, double x0) { return 2.0 * xn - x0; }

template <int LV>
DOPF_CS_FN void cs_reduced_costs(const StoRow &r, double pi, double suf, double &rD, double &rC)
{
    if constexpr (LV == 3) { rD = r.mc + pi - r.al * suf; rC = r.mc - pi + r.be * suf; }
    else { rD = r.mc + pi - suf; rC = r.mc - pi + suf; }
}

// D+, C+ of column t at primal weight w
template <int LV>
DOPF_CS_FN void cs_column_steps(const StoRow &r, double absH, double w, int T, int t, double d0, double c0, double rD, double rC,
                                double &dn, double &cn)
{
    if constexpr (LV == 3) {
        const double tauD = 1.0 / ((1.0 + absH + r.al * (double)(T - t)) * w);
        const double tauC = 1.0 / ((1.0 + absH + r.be * (double)(T - t)) * w);
        dn = cs_clamp(d0 - tauD * rD, 0.0, r.pm);
        cn = cs_clamp(c0 - tauC * rC, 0.0, r.pm);
    } else {
        const double tau = 1.0 / ((1.0 + absH + (double)(T - t)) * w);
        dn = cs_clamp(d0 - tau * rD, 0.0, r.pm);
        cn = cs_clamp(c0 - tau * rC, 0.0, r.pm);
    }
}

// what (d, c) adds to the level
template <int LV>
DOPF_CS_FN double cs_net(const StoRow &r, double d, double c)
{
    if constexpr (LV == 3) return r.be * c - r.al * d;
    else return c - d;
}

// the row's step size: w over its sum of |K|, (al + be) (t + 1)
template <int LV>
DOPF_CS_FN double cs_sigma(const StoRow &r, double w, int t)
{
    if constexpr (LV == 3) return w / ((r.al + r.be) * (double)(t + 1));
    else return w / (2.0 * (double)(t + 1));
}

template <int LV>
DOPF_CS_FN double cs_lb(const StoRow &r, int t, int T)
{
    if constexpr (LV >= 2) return t == T - 1 ? r.elo : 0.0;
    else return 0.0;
}

template <int LV>
DOPF_CS_FN double cs_ub(const StoRow &r, int t, int T)
{
    if constexpr (LV >= 2) return t == T - 1 ? r.ehi : r.em;
    else return r.em;
}

// y+ of row t from z = y + sigma level: the proximal step of the support function of [lb_t, ub_t] — written in the level, which includes
// e0 (the row sum_{tau <= t} (be C - al D) onto [lb_t - e0, ub_t - e0]: the same step, e0 moved to the other side)
template <int LV>
DOPF_CS_FN double cs_prox(const StoRow &r, double z, double sigma, int t, int T)
{
    return z - sigma * cs_clamp(z / sigma, cs_lb<LV>(r, t, T), cs_ub<LV>(r, t, T));
}

// the column pair's term of the dual objective: min over the boxes [0, pm] of rD d + rC c
DOPF_CS_FN double cs_rc_term(double rD, double rC, double pm) { return (__builtin_fmin(rD, 0.0) + __builtin_fmin(rC, 0.0)) * pm; }

// sum + max(y, 0) (ub_t - e0) + min(y, 0) (lb_t - e0), the interval's support function (the caller subtracts the sum). From LV 1 on two
// fused steps, the first the one LV 0's product and sum become on the device: with e0 = 0 and the default band the same bits there. A
// host build without contraction rounds LV 0's product and its sum separately.
template <int LV>
DOPF_CS_FN double cs_support(const StoRow &r, double y, int t, int T, double sum)
{
    if constexpr (LV == 0) return sum + __builtin_fmax(y, 0.0) * r.em;
    else {
        sum = __builtin_fma(__builtin_fmax(y, 0.0), cs_ub<LV>(r, t, T) - r.e0, sum);
        return __builtin_fma(__builtin_fmin(y, 0.0), cs_lb<LV>(r, t, T) - r.e0, sum);
    }
}

// how far the level lies outside [lb_t, ub_t] (negative inside: the caller's running maximum starts at 0)
template <int LV>
DOPF_CS_FN double cs_violation(const StoRow &r, double lev, int t, int T)
{
    if constexpr (LV >= 2) return __builtin_fmax(cs_lb<LV>(r, t, T) - lev, lev - cs_ub<LV>(r, t, T));
    else return __builtin_fmax(-lev, lev - r.em);
}

}  // namespace dopf
