// ramp_price.h — the multipliers of a generator row's ramp rows (dopf_get_generator_ramp_price), read off the STORED
// row and its centres, not off the dynamic programme that repaired it. Plain C++, no HIP include: lane 0 of the wave that owns a
// repaired row runs it in k_gen_ramp<.., RP = true> and k_gen_ramp_budget<.., RP = true>, tests/ramp_price_main.cpp as a host program
// under sanitizers.
//
// A repaired row x is the exact minimiser of sum_t q/2 (x_t - c_t)^2 over {floor_t <= x_t <= cap_t, ramps, anchor}. Its multipliers
// solve the chain a_{t+1} = a_t + g_t + b_t, a_T = 0, with g_t = q (x_t - c_t): a_t the net multiplier of the ramp row between t-1
// and t (t = 0: the anchor's row; >= 0 where ramp-up is tight, <= 0 where ramp-down is, 0 otherwise), b_t the box's (>= 0 at the cap,
// <= 0 at the floor, 0 inside, free where floor = cap). The feasible a_t form intervals: one forward pass of intervals A_t and one
// backward pick give a valid vector in O(T).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_RP_FN __host__ __device__ inline
#else
#define DOPF_RP_FN inline
#endif

namespace dopf {

DOPF_RP_FN double rp_min(double a, double b) { return a < b ? a : b; }      // (operands are never NaN here)
DOPF_RP_FN double rp_max(double a, double b) { return a > b ? a : b; }

// g_t = q (x_t - (c_t - shift)): one rounded product, never contracted into the additions behind it (as avail_mul's)
DOPF_RP_FN double rp_grad(double q, double x, double c, double shift)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double g = q * (x - (c - shift));
    return g;
}

// near(I, S): I ∩ S, or where that is empty the end of S nearest to I (one point); I = [il, ih] in and out
DOPF_RP_FN void rp_near(double &il, double &ih, double sl, double sh)
{
    const double l = rp_max(il, sl), h = rp_min(ih, sh);
    if (l <= h) { il = l; ih = h; }
    else if (ih < sl) il = ih = sl;
    else il = ih = sh;
}

// The pass. x: the stored row, c: its centres (the row's step is the projection of c_t - shift; shift = nu / q under a budget
// multiplier nu, else 0), floor(t) / cap(t): the box of step t, up / down: the STORED ramps, not capped at pm — an infinite ramp is
// never tight —, prev: the anchor (NaN: none, S_0 = {0}), pm: gen_pmax[g], which scales the tolerance: the programme reaches x_t as
// y + up and x_{t-1} as x_t - up, an ulp apart, so exact comparisons would miss tight rows; a false "tight" only widens a set that
// still holds the true multipliers. lo, hi: T doubles each of work (the intervals A_t). a: T values out, a[t] = the multiplier of the
// row between t-1 and t, the point nearest 0 where the multipliers are not unique. a may be c itself: c_t is read before a_t is stored.
template <class Floor, class Cap>
DOPF_RP_FN void ramp_price(const double *x, const double *c, double shift, double q, const Floor &floor, const Cap &cap, int T,
                           double up, double down, double prev, double pm, double *lo, double *hi, double *a)
{
    const double tol = pm * 0x1p-40, inf = __builtin_inf();
    double al = 0.0, ah = 0.0;
    for (int t = 0; t < T; ++t) {
        const double xt = x[t], before = t ? x[t - 1] : prev;
        double sl = 0.0, sh = 0.0;
        if (before == before) {
            if (before - xt >= down - tol) sl = -inf;
            if (xt - before >= up - tol) sh = inf;
        }
        if (t == 0) { al = sl; ah = sh; }
        else rp_near(al, ah, sl, sh);
        lo[t] = al; hi[t] = ah;
        const double g = rp_grad(q, xt, c[t], shift);
        const double bl = xt <= floor(t) + tol ? -inf : 0.0, bh = xt >= cap(t) - tol ? inf : 0.0;
        al = (al + g) + bl;
        ah = (ah + g) + bh;
    }
    double an = 0.0;                                // a_T = 0: no row behind the last step
    for (int t = T - 1; t >= 0; --t) {
        const double xt = x[t];
        const double g = rp_grad(q, xt, c[t], shift);
        const double bl = xt <= floor(t) + tol ? -inf : 0.0, bh = xt >= cap(t) - tol ? inf : 0.0;
        double l = (an - g) - bh, h = (an - g) - bl;
        rp_near(l, h, lo[t], hi[t]);
        an = rp_min(rp_max(0.0, l), h);
        a[t] = an;
    }
}

}  // namespace dopf
