// gen_ramp.h — DOPF_F_GEN_RAMP (copper plates): the generators' x-update under ramp limits, a launch of its own.
// Included by kernels_agents.hip behind its kernels (it uses that file's clampd and the helpers of dopf_internal.h).
//
// Row g keeps its separable quadratic objective and its box 0 <= P[g,t] <= cap[g,t] and gains
//     -down <= P[g,t] - P[g,t-1] <= up (t >= 1),   -down <= P[g,0] - prev <= up (anchored rows),
// so its step is the Euclidean projection of c, c_t = the unclamped step of gen_update_body, onto {box, ramps}.
// With floors (dopf_set_generator_min_output; the MN instantiations) the box is fmin(p_min[g], cap[g,t]) <= P[g,t] <= cap[g,t].
//
// One block per generator item, kRampWaves waves, in three phases:
//  1. a wave per row, lanes over t (P is agent-major: a row's T values are consecutive, the wave's loads and stores are whole
//     lines): the clamped step of k_gen_update<false, AV, QC>, bit for bit, is stored, c_t is kept (LDS up to T = kRampLdsT, the
//     wave's scratch behind gen_pmax beyond) and every difference of neighbours is held against the ramps;
//  2. a row whose clamped step keeps its ramps is optimal and done (the settled case). For the others lane 0 of the wave solves the
//     projection exactly (ramp_repair): O(T x knots), knots <= 2T + 2, serial — the price of a row that leaves the fast path;
//  3. the item's sums from the stored rows, in k_gen_update's order with k_gen_update's tiling: the same bits whenever the rows are.
#pragma once

#include "ramp_price.h"

namespace dopf {

// the box of step t as ramp_price (ramp_price.h) takes it: cap_t, and the floor fmin(p_min, cap_t) (MN) or 0
template <bool AV>
struct RampCap {
    const double *ftab;
    double pm;
    int T, prof;
    __device__ __forceinline__ double operator()(int t) const { return AV ? avail_cap(ftab, T, prof, pm, t) : pm; }
};
template <bool AV, bool MN>
struct RampFloor {
    RampCap<AV> cap;
    double pmn;
    __device__ __forceinline__ double operator()(int t) const { return MN ? fmin(pmn, cap(t)) : 0.0; }
};

// h'(x) between two knots (xa <= x <= xb); equal values need no slope (and no finite xb - xa)
__device__ __forceinline__ double ramp_interp(double xa, double va, double xb, double vb, double x)
{
    return va == vb ? va : va + (x - xa) * ((vb - va) / (xb - xa));
}

// the smallest x with h'(x) >= 0, clamped to the knots' range (n >= 1 knots, v non-decreasing; two knots may share an x: a jump)
__device__ __forceinline__ double ramp_argmin(const double *kx, const double *kv, int n)
{
    int k = 0;
    while (k < n && kv[k] < 0.0) ++k;
    if (k == 0) return kx[0];
    if (k == n) return kx[n - 1];
    const double xa = kx[k - 1], va = kv[k - 1], xb = kx[k], vb = kv[k];
    if (xb == xa) return xb;
    return clampd(xa + (-va) * ((xb - xa) / (vb - va)), xa, xb);
}

// The exact projection of one row, by one lane. Forward: h_t', the derivative of the cost-to-go as a function of x_t, non-decreasing
// and piecewise linear, as knots (kx, kv) — per step: y*_{t-1} = argmin h_{t-1}; the knots with v < 0 move down by `down`, those
// with v > 0 up by `up` (split by the SIGN of v, which keeps a jump's one-sided values), v == 0 goes, (y* - down, 0) and (y* + up, 0)
// come between; clip to [0, cap_t]; add q (x - c_t). At most two knots more per step: n <= 2T. Backward: P[T-1] = y*_{T-1},
// P[t-1] = clamp(y*_{t-1}, P[t] - up, P[t] + down). cy holds c_t on entry, y*_t behind the step that used c_t.
// up, down: finite (the caller caps them at pmax: a ramp of pmax or more never binds inside [0, pmax]).
// MN (dopf_set_generator_min_output): the box of step t is [fmin(pmn, cap_t), cap_t] — a floor that follows the cap down
// — in [0, cap_t]'s place; the setter has made sure that a path exists.
template <bool AV, bool MN = false>
__device__ __forceinline__ void ramp_repair(double *Prow, double *cy, double *kx, double *kv, int T, double q, double up, double down,
                                         double prev, double pm, const double *ftab, int prof, double pmn = 0.0)
{
    double lo = 0.0, hi = AV ? avail_cap(ftab, T, prof, pm, 0) : pm;
    if constexpr (MN) lo = fmin(pmn, hi);
    if (prev == prev) { lo = fmax(lo, prev - down); hi = fmin(hi, prev + up); }
    hi = fmax(hi, lo);
    kx[0] = lo; kv[0] = q * (lo - cy[0]);
    kx[1] = hi; kv[1] = q * (hi - cy[0]);
    int n = 2;
    for (int t = 1; t < T; ++t) {
        const double y = ramp_argmin(kx, kv, n);
        cy[t - 1] = y;
        int k = 0, p;                               // [0, k): v < 0; [p, n): v > 0
        while (k < n && kv[k] < 0.0) ++k;
        p = k;
        while (p < n && kv[p] <= 0.0) ++p;
        // the suffix to [k + 2, ..) moved up by `up`, in the direction that overwrites nothing unread
        const int sh = k + 2 - p, n2 = k + 2 + (n - p);
        if (sh > 0) for (int j = n - 1; j >= p; --j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        else for (int j = p; j < n; ++j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        for (int j = 0; j < k; ++j) kx[j] -= down;
        kx[k] = y - down; kv[k] = 0.0;
        kx[k + 1] = y + up; kv[k + 1] = 0.0;
        // clip to [lo, hi]: the value at lo from the right (the last knot at or below it), at hi from the left (the first at or above)
        const double cap = AV ? avail_cap(ftab, T, prof, pm, t) : pm;
        if constexpr (MN) lo = fmax(fmin(pmn, cap), kx[0]);
        else lo = fmax(0.0, kx[0]);
        hi = fmax(fmin(cap, kx[n2 - 1]), lo);
        int a = 0, b = n2 - 1;
        while (a + 1 < n2 && kx[a + 1] <= lo) ++a;
        while (b > 0 && kx[b - 1] >= hi) --b;
        double vlo = kx[a] == lo ? kv[a] : ramp_interp(kx[a], kv[a], kx[a + 1], kv[a + 1], lo);
        double vhi = kx[b] == hi ? kv[b] : ramp_interp(kx[b - 1], kv[b - 1], kx[b], kv[b], hi);
        if (!(lo < hi)) vlo = vhi = 0.0;             // one point: nothing of h' is left
        const double c = cy[t];
        int m = 1;
        for (int j = a + 1; j < b; ++j, ++m) {      // (m <= j: ascending copies overwrite nothing unread)
            const double x = kx[j];
            kv[m] = kv[j] + q * (x - c);
            kx[m] = x;
        }
        kx[0] = lo; kv[0] = vlo + q * (lo - c);
        kx[m] = hi; kv[m] = vhi + q * (hi - c);
        n = m + 1;
    }
    double pn = ramp_argmin(kx, kv, n);
    Prow[T - 1] = pn;
    for (int t = T - 1; t > 0; --t) {
        pn = clampd(cy[t - 1], pn - up, pn + down);
        Prow[t - 1] = pn;
    }
}

// MN: the rows' floors (gen_min_output(v)) are read and the box is [fmin(p_min, cap), cap]; the MN = false instantiations are the
// kernels of the contexts that never set a floor.
// RP (dopf_get_generator_ramp_price): the rows' ramp multipliers go into rpv, T doubles per row in sorted order — zeros
// for a row that needs no repair (lanes over t: whole lines); for a repaired row the wave copies its centres there before ramp_repair
// overwrites them, and lane 0 runs ramp_price behind the repair, in place over them, its intervals in the row's kx / kv, which are
// free by then. RP = false (rpv unused) is the code of before: what a context runs until its first call of that entry
template <bool AV, bool QC, bool MN, bool RP>
__global__ __launch_bounds__(512) void k_gen_ramp(DevView v, double *rpv)
{
    if (v.st->halt) return;
    constexpr int NK = 2 * kRampLdsT + 2;
    __shared__ double red[512];
    __shared__ double s_cy[kRampWaves][kRampLdsT], s_kx[kRampWaves][NK], s_kv[kRampWaves][NK];
    const Item it = v.gen_items[blockIdx.x];
    const int T = v.T, N = v.N;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double w = v.w_prox, gam = v.gamma;
    const double inv = 1.0 / (w + gam);
    const double *ftab = nullptr;
    const int *prof = nullptr;
    if constexpr (AV) { ftab = *gen_avail_slot(v); prof = gen_prof(v); }
    const double *c2v = nullptr;
    if constexpr (QC) c2v = gen_c2(v);
    const double *upv = gen_ramp_up(v), *dnv = gen_ramp_down(v), *pvv = gen_ramp_prev(v);
    const double *mnv = nullptr;
    if constexpr (MN) mnv = gen_min_output(v);

    // the wave's c_t / y*_t and knots: LDS, or (long horizons) its scratch behind gen_pmax
    double *cy = s_cy[wave], *kx = s_kx[wave], *kv = s_kv[wave];
    if (T > kRampLdsT) {
        cy = gen_ramp_scratch(v) + ((size_t)blockIdx.x * kRampWaves + wave) * ramp_row_doubles(T);
        kx = cy + T;
        kv = kx + 2 * (size_t)T + 2;
    }

    for (int g = it.a0 + wave; g < it.a1; g += kRampWaves) {
        const double mc = v.gen_mc[g], pm = v.gen_pmax[g];
        const double up = upv[g], dn = dnv[g], prev = pvv[g];
        const int pr = AV ? prof[g] : -1;
        double c2 = 0.0, iq = inv, pmn = 0.0;
        if constexpr (QC) { c2 = c2v[g]; iq = 1.0 / ((w + gam) + c2); }
        if constexpr (MN) pmn = mnv[g];
        double *Prow = v.P + (size_t)g * T;
        double left = prev;                         // the value in front of the chunk's first timestep (NaN: none)
        bool bad = false;
        for (int tc = 0; tc < T; tc += 64) {
            const int t = tc + lane;
            double pn = 0.0;
            if (t < T) {
                // copper plate: Psi(d) = price + gamma (s + d) — the expressions of gen_update_body, LINES = false
                const double psum = v.price[it.node + N * t] + gam * v.s[t];
                const double p0 = Prow[t];
                double c;
                if constexpr (QC) c = p0 - fma(mc + c2 * p0, iq, psum * iq);
                else c = p0 - fma(mc, inv, psum * inv);       // (mc * inv + shift as gen_update_body's loop contracts it)
                if constexpr (MN) {
                    const double cap = AV ? avail_cap(ftab, T, pr, pm, t) : pm;
                    pn = clampd(c, fmin(pmn, cap), cap);
                } else {
                    pn = clampd(c, 0.0, AV ? avail_cap(ftab, T, pr, pm, t) : pm);
                }
                Prow[t] = pn;
                cy[t] = c;
            }
            double before = __shfl_up(pn, 1);
            if (lane == 0) before = left;
            if (t < T && before == before) {
                const double d = pn - before;
                bad = bad || d > up || -d > dn;
            }
            left = __shfl(pn, 63);
        }
        if constexpr (RP) {
            double *rrow = rpv + (size_t)g * T;
            if (__any(bad)) {
                __threadfence_block();              // the wave's c_t, before the wave reads them
                for (int t = lane; t < T; t += 64) rrow[t] = cy[t];
                __threadfence_block();              // ... and their copy, before lane 0 does
                if (lane == 0) {
                    ramp_repair<AV, MN>(Prow, cy, kx, kv, T, (w + gam) + c2, fmin(up, pm), fmin(dn, pm), prev, pm, ftab, pr, pmn);
                    // the stored ramps: an infinite one is never tight. T <= kRampLdsT or the scratch's 2T + 2: room for T intervals
                    const RampCap<AV> cap{ftab, pm, T, pr};
                    ramp_price(Prow, rrow, 0.0, (w + gam) + c2, RampFloor<AV, MN>{cap, pmn}, cap, T, up, dn, prev, pm, kx, kv, rrow);
                }
                __threadfence_block();
            } else {
                for (int t = lane; t < T; t += 64) rrow[t] = 0.0;
            }
        } else if (__any(bad)) {
            __threadfence_block();                  // the wave's c_t, before lane 0 reads them
            if (lane == 0)
                ramp_repair<AV, MN>(Prow, cy, kx, kv, T, (w + gam) + c2, fmin(up, pm), fmin(dn, pm), prev, pm, ftab, pr, pmn);
            __threadfence_block();
        }
    }
    __syncthreads();

    // the item's sums, from the rows as stored: k_gen_update's tiling and order of additions
    const int TT = v.genTT, R = v.genR;
    const int r = tid / TT, tt = tid - r * TT;
    double cost = 0.0;
    for (int tc = 0; tc < T; tc += TT) {
        const int t = tc + tt;
        double acc = 0.0;
        if (r < R && t < T) {
#pragma unroll 4
            for (int g = it.a0 + r; g < it.a1; g += R) {
                const double mc = v.gen_mc[g];
                const double pn = v.P[(size_t)g * T + t];
                acc += pn;
                cost += mc * pn;
                if constexpr (QC) cost += (0.5 * c2v[g] * pn) * pn;
            }
        }
        red[tid] = acc;
        __syncthreads();
        if (r == 0 && t < T) {
            double sum = 0.0;
            for (int q = 0; q < R; ++q) sum += red[q * TT + tt];
            v.part_ginj[(size_t)blockIdx.x * T + t] = sum;
        }
        __syncthreads();
    }
    __shared__ double wcost[8];
    for (int d = 32; d > 0; d >>= 1) cost += __shfl_xor(cost, d);
    if ((tid & 63) == 0) wcost[tid >> 6] = cost;
    __syncthreads();
    if (tid == 0) {
        double c = 0.0;
        for (int q = 0; q < 8; ++q) c += wcost[q];
        v.part_gcost[blockIdx.x] = c;
    }
}

void launch_gen_ramp(const DevView &v, const Plan &p, hipStream_t s)
{
    if (v.nGenItems == 0) return;
    with_bool(p.genAvail, [&](auto av) {
        with_bool(p.genQuad, [&](auto qc) {
            with_bool(p.genMinOut, [&](auto mn) {
                with_bool(p.genRampPrice != nullptr, [&](auto rp) {
                    hipLaunchKernelGGL((k_gen_ramp<decltype(av)::value, decltype(qc)::value, decltype(mn)::value, decltype(rp)::value>),
                                       dim3(v.nGenItems), dim3(512), 0, s, v, p.genRampPrice);
                });
            });
        });
    });
}

}  // namespace dopf
