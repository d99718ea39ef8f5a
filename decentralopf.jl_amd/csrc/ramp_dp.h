// ramp_dp.h — the exact generator step under ramp limits where a step's derivative is piecewise linear (DOPF_F_GEN_RAMP_NETWORK,
// DESIGN.md 5s): the dynamic programme of DESIGN.md 5r with the kinks of the node's Psi merged into the knots of the cost-to-go.
// Plain C++, no HIP include: gen_ramp_net.h runs it on one lane per repaired row, tests/ramp_net_main.cpp as a host program under
// sanitizers; tests/helpers_ramp_net.ramp_project_pwl is the same programme in NumPy, statement by statement.
//
// Row g minimises sum_t f_t(x_t) over 0 <= x_t <= cap_t, -down <= x_t - x_{t-1} <= up (t >= 1; t = 0 against prev where one is given),
// f_t convex with the continuous, increasing, piecewise-linear derivative phi_t. A step type describes phi_t:
//     int m() const              kinks of phi_t (0: one line)
//     double kink(int j) const   their x, ascending (j < m)
//     double phi(double x, int &piece) const   phi_t(x); piece: a cursor that only moves up while x does (start it at 0)
// and a row type hands out cap(t) and step(t) — and, only where ramp_repair_pwl is asked for floors (FLOOR), floor(t) <= cap(t): the
// box of step t is then floor(t) <= x_t <= cap(t) (dopf_set_generator_min_output).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_DP_FN __device__ __forceinline__
#define DOPF_DP_HD __host__ __device__ inline
#else
#define DOPF_DP_FN inline
#define DOPF_DP_HD inline
#endif

#include <stddef.h>

namespace dopf {

// Knot capacity of a row in flight on a network: 2T + 2 from the ramps and one per kink of Psi that falls inside the
// row's reach, sum_t m_t <= 2 L T — bounded by kRampNetKinks, a sizing choice (configs[3] at full size stays under
// 1 GiB of scratch), not a measurement. A row that needs more fails (ramp_repair_pwl returns false).
constexpr int kRampNetKinks = 4096;
DOPF_DP_HD int ramp_net_knots(int T, int L)
{
    const long long kinks = 2ll * L * T;
    return 2 * T + 2 + (int)(kinks < kRampNetKinks ? kinks : kRampNetKinks);
}
// a wave's scratch: p0[T] | y*[T] | kx[K] | kv[K]
DOPF_DP_HD size_t ramp_net_row_doubles(int T, int L) { return 2 * (size_t)T + 2 * (size_t)ramp_net_knots(T, L); }

DOPF_DP_FN double dp_min(double a, double b) { return a < b ? a : b; }      // (operands are never NaN here)
DOPF_DP_FN double dp_max(double a, double b) { return a > b ? a : b; }

// h'(x) between two knots (xa <= x <= xb); equal values need no slope (and no finite xb - xa)
DOPF_DP_FN double dp_interp(double xa, double va, double xb, double vb, double x)
{
    return va == vb ? va : va + (x - xa) * ((vb - va) / (xb - xa));
}

// the smallest x with h'(x) >= 0, clamped to the knots' range (n >= 1 knots, v non-decreasing; two knots may share an x: a jump)
DOPF_DP_FN double dp_argmin(const double *kx, const double *kv, int n)
{
    int k = 0;
    while (k < n && kv[k] < 0.0) ++k;
    if (k == 0) return kx[0];
    if (k == n) return kx[n - 1];
    const double xa = kx[k - 1], va = kv[k - 1], xb = kx[k], vb = kv[k];
    if (xb == xa) return xb;
    return dp_min(dp_max(xa + (-va) * ((xb - xa) / (vb - va)), xa), xb);
}

// phi_t as absolute knots: kinks xk[j] with values vk[j] = phi(xk[j]) and the slopes sl[0 .. m] of the m + 1 pieces; m == 0: one line
// of slope sl[0] through (xk[0], vk[0]). On piece p the value is taken from kink min(p, m - 1): vk[a] + sl[p] (x - xk[a]).
struct RampStepPwl {
    int mm;
    const double *xk, *vk, *sl;
    DOPF_DP_FN int m() const { return mm; }
    DOPF_DP_FN double kink(int j) const { return xk[j]; }
    DOPF_DP_FN double phi(double x, int &piece) const
    {
        while (piece < mm && xk[piece] < x) ++piece;
        const int a = piece < mm ? piece : (mm > 0 ? mm - 1 : 0);
        return vk[a] + sl[piece] * (x - xk[a]);
    }
};

// phi_t(x) = mc + c2 x + Psi(x - p0) + w (x - p0) from the table of the node's Psi at one timestep (beta, psi, slope, psi0, m as
// k_tables leaves them: Psi(d) = psi[a] + slope[piece] (d - beta[a]), a = min(piece, m - 1); m == 0: psi0 + slope[0] d). m == 0 is the
// copper-plate step with a q of its own: q (x - c), q = slope[0] + w + c2, c = p0 - (mc + c2 p0 + psi0) / q.
struct RampStepTab {
    int mm;
    const double *beta, *psi, *slope;
    double psi0, p0, mc, c2, w;
    DOPF_DP_FN int m() const { return mm; }
    DOPF_DP_FN double kink(int j) const { return p0 + beta[j]; }
    DOPF_DP_FN double phi(double x, int &piece) const
    {
        if (mm == 0) {
            const double q = slope[0] + w + c2;
            return q * (x - (p0 - (mc + c2 * p0 + psi0) / q));
        }
        const double d = x - p0;
        while (piece < mm && beta[piece] < d) ++piece;
        const int a = piece < mm ? piece : mm - 1;
        return (mc + c2 * x) + (psi[a] + slope[piece] * (d - beta[a])) + w * d;
    }
};

// Step (4) of the programme: phi's kinks strictly inside (kx[0], kx[n - 1]) become knots — a backward merge in place, both lists are
// sorted; a new knot's value is interpolated between the old knot at or left of it and whatever already stands right of it — then
// phi is added at every knot. Returns the new count, or -1, with nothing written, where it would exceed K.
template <class Step>
DOPF_DP_FN int dp_add_phi(const Step &st, double *kx, double *kv, int n, int K)
{
    const int m = st.m();
    if (m > 0) {
        const double lo = kx[0], hi = kx[n - 1];
        int j0 = 0, j1;
        while (j0 < m && !(st.kink(j0) > lo)) ++j0;
        j1 = j0;
        while (j1 < m && st.kink(j1) < hi) ++j1;
        const int cnt = j1 - j0;
        if (n + cnt > K) return -1;
        int i = n - 1, w = n + cnt - 1;
        for (int j = j1 - 1; j >= j0; --w) {
            const double x = st.kink(j);
            if (kx[i] > x) {
                kx[w] = kx[i]; kv[w] = kv[i];
                --i;
            } else {
                kv[w] = dp_interp(kx[i], kv[i], kx[w + 1], kv[w + 1], x);
                kx[w] = x;
                --j;
            }
        }
        n += cnt;
    }
    int piece = 0;
    for (int k = 0; k < n; ++k) kv[k] += st.phi(kx[k], piece);
    return n;
}

// The exact step of one row, serially. Forward: h_t', the derivative of the cost-to-go as a function of x_t, non-decreasing and
// piecewise linear, as knots (kx, kv) of capacity K — per step: y*_{t-1} = argmin h_{t-1}; the knots with v < 0 move down by `down`,
// those with v > 0 up by `up` (split by the SIGN of v, which keeps a jump's one-sided values), v == 0 goes, (y* - down, 0) and
// (y* + up, 0) come between; clip to [0, cap_t]; add phi_t (dp_add_phi). Backward: x[T-1] = y*_{T-1},
// x[t-1] = clamp(y*_{t-1}, x[t] - up, x[t] + down). cy: T doubles of scratch (y*_t). up, down: finite (the caller caps them at the
// row's largest cap: such a ramp never binds). prev: NaN = no anchor. Returns false — out (T values) untouched, nothing written
// beyond kx[K - 1], kv[K - 1] — where the knots would exceed K. FLOOR: the lower end of step t's box is row.floor(t) in 0's place
// (a row type without floor() serves the default; the caller has made sure that a path exists: dopf_set_generator_min_output).
template <bool FLOOR = false, class Row>
DOPF_DP_FN bool ramp_repair_pwl(const Row &row, double *out, double *cy, double *kx, double *kv, int K, int T, double up, double down,
                                double prev)
{
    if (K < 2) return false;
    double lo = 0.0, hi = row.cap(0);
    if constexpr (FLOOR) lo = row.floor(0);
    if (prev == prev) { lo = dp_max(lo, prev - down); hi = dp_min(hi, prev + up); }
    hi = dp_max(hi, lo);
    kx[0] = lo; kv[0] = 0.0;
    kx[1] = hi; kv[1] = 0.0;
    int n = dp_add_phi(row.step(0), kx, kv, 2, K);
    if (n < 0) return false;
    for (int t = 1; t < T; ++t) {
        const double y = dp_argmin(kx, kv, n);
        cy[t - 1] = y;
        int k = 0, p;                               // [0, k): v < 0; [p, n): v > 0
        while (k < n && kv[k] < 0.0) ++k;
        p = k;
        while (p < n && kv[p] <= 0.0) ++p;
        // the suffix to [k + 2, ..) moved up by `up`, in the direction that overwrites nothing unread
        const int sh = k + 2 - p, n2 = k + 2 + (n - p);
        if (n2 > K) return false;
        if (sh > 0) for (int j = n - 1; j >= p; --j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        else for (int j = p; j < n; ++j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        for (int j = 0; j < k; ++j) kx[j] -= down;
        kx[k] = y - down; kv[k] = 0.0;
        kx[k + 1] = y + up; kv[k + 1] = 0.0;
        // clip to [lo, hi]: the value at lo from the right (the last knot at or below it), at hi from the left (the first at or above)
        if constexpr (FLOOR) lo = dp_max(row.floor(t), kx[0]);
        else lo = dp_max(0.0, kx[0]);
        hi = dp_max(dp_min(row.cap(t), kx[n2 - 1]), lo);
        int a = 0, b = n2 - 1;
        while (a + 1 < n2 && kx[a + 1] <= lo) ++a;
        while (b > 0 && kx[b - 1] >= hi) --b;
        double vlo = kx[a] == lo ? kv[a] : dp_interp(kx[a], kv[a], kx[a + 1], kv[a + 1], lo);
        double vhi = kx[b] == hi ? kv[b] : dp_interp(kx[b - 1], kv[b - 1], kx[b], kv[b], hi);
        if (!(lo < hi)) vlo = vhi = 0.0;             // one point: nothing of h' is left
        int m = 1;
        for (int j = a + 1; j < b; ++j, ++m) {      // (m <= j: ascending copies overwrite nothing unread)
            kv[m] = kv[j];
            kx[m] = kx[j];
        }
        kx[0] = lo; kv[0] = vlo;
        kx[m] = hi; kv[m] = vhi;
        n = dp_add_phi(row.step(t), kx, kv, m + 1, K);
        if (n < 0) return false;
    }
    double pn = dp_argmin(kx, kv, n);
    out[T - 1] = pn;
    for (int t = T - 1; t > 0; --t) {
        pn = dp_min(dp_max(cy[t - 1], pn - up), pn + down);
        out[t - 1] = pn;
    }
    return true;
}

}  // namespace dopf
