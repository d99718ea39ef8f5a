// ramp_budget.h — a generator row under ramp limits AND an energy budget (DOPF_F2_GEN_RAMP_BUDGET): the ramp programme
// of DESIGN.md 5r inside the one-multiplier search of DESIGN.md 5t. Plain C++, no HIP include: gen_ramp_budget.h runs it with a
// candidate per lane of the wave that owns the row, tests/ramp_budget_main.cpp as a host program under sanitizers.
//
// With a multiplier nu on the budget row the row's step is x(nu), the projection of the centres c_t - nu / q onto {box, ramps}
// (q = w_prox + gamma + c2). x(nu) is the projection of a line onto a polytope: continuous and piecewise linear, and
// phi(nu) = sum_t x_t(nu) is non-increasing. The preimage of a face's relative interior under a projection is convex, so two
// candidates with the same active set bracket a stretch on which x is affine: one division gives the root. The active set is read off
// the branches the programme takes (ramp_budget_run's signature), never off differences formed again in floating point.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_RB_FN __host__ __device__ inline
#define DOPF_RB_NOUNROLL _Pragma("nounroll")        // (the scans over a batch are shuffles on the device: 64 copies of one would only cost registers)
#else
#define DOPF_RB_FN inline
#define DOPF_RB_NOUNROLL
#endif

namespace dopf {

// rounds (batches of candidates) a row may spend before it gives up: the first brackets the root on a geometric grid, every later one
// cuts the bracket to a 65th (ten of them leave no double), a secant point that misses its check costs one more
constexpr int kRampBudgetMaxRounds = 32;
constexpr int kRampBudgetLanes = 64;        // candidates per batch: a wave's lanes

// element i of a lane's array in the interleaved [slot][lane] layout (stride 64 on the device, 1 on the host)
struct RbSpan {
    double *p;
    size_t s;
    DOPF_RB_FN double &operator[](int i) const { return p[(size_t)i * s]; }
};

DOPF_RB_FN double rb_min(double a, double b) { return a < b ? a : b; }      // (operands are never NaN here)
DOPF_RB_FN double rb_max(double a, double b) { return a > b ? a : b; }

DOPF_RB_FN double rb_interp(double xa, double va, double xb, double vb, double x)
{
    return va == vb ? va : va + (x - xa) * ((vb - va) / (xb - xa));
}

// ramp_argmin (gen_ramp.h) with its branch: 0 the first knot, 1 the last, 2 between
template <class A>
DOPF_RB_FN double rb_argmin(const A &kx, const A &kv, int n, int &branch)
{
    int k = 0;
    while (k < n && kv[k] < 0.0) ++k;
    if (k == 0) { branch = 0; return kx[0]; }
    if (k == n) { branch = 1; return kx[n - 1]; }
    branch = 2;
    const double xa = kx[k - 1], va = kv[k - 1], xb = kx[k], vb = kv[k];
    if (xb == xa) return xb;
    return rb_min(rb_max(xa + (-va) * ((xb - xa) / (vb - va)), xa), xb);
}

DOPF_RB_FN unsigned long long rb_fold(unsigned long long sig, unsigned code) { return (sig ^ (unsigned long long)code) * 1099511628211ull; }

// The programme of ramp_repair (gen_ramp.h), statement by statement, for the centres c[t] - shift, with the sum of its row and the
// signature of its active set. Per timestep the signature takes the branch of y*'s argmin, the sides of the clip (the box's end or
// the reach of the ramps, on either side; the anchor's at t = 0) and the one-point case, in the backward pass the side of
// clamp(y*, x - up, x + down) and whether the value sits on an end of its box. cap(t): the row's upper bound. y (T), kx, kv (K each,
// K >= 2T + 2): the lane's work arrays. out: null, or T values (the row). up, down: finite. prev: NaN = no anchor.
// Returns false, with nothing of out written, where the knots would exceed K (the bound of DESIGN.md 5r says they do not).
template <class A, class Cap>
DOPF_RB_FN bool ramp_budget_run(const double *c, double shift, const Cap &cap, int T, double q, double up, double down, double prev,
                                const A &y, const A &kx, const A &kv, int K, double *out, double *sum, unsigned long long *sig)
{
    unsigned long long sg = 14695981039346656037ull;
    if (K < 2) return false;
    double lo = 0.0, hi = cap(0);
    unsigned code = 0;
    if (prev == prev) {
        if (prev - down > lo) { lo = prev - down; code |= 1u; }
        if (prev + up < hi) { hi = prev + up; code |= 2u; }
    }
    if (hi < lo) { hi = lo; code |= 4u; }
    sg = rb_fold(sg, code);
    const double c0 = c[0] - shift;
    kx[0] = lo; kv[0] = q * (lo - c0);
    kx[1] = hi; kv[1] = q * (hi - c0);
    int n = 2, br;
    for (int t = 1; t < T; ++t) {
        const double ys = rb_argmin(kx, kv, n, br);
        y[t - 1] = ys;
        int k = 0, p;                               // [0, k): v < 0; [p, n): v > 0
        while (k < n && kv[k] < 0.0) ++k;
        p = k;
        while (p < n && kv[p] <= 0.0) ++p;
        const int sh = k + 2 - p, n2 = k + 2 + (n - p);
        if (n2 > K) return false;
        if (sh > 0) for (int j = n - 1; j >= p; --j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        else for (int j = p; j < n; ++j) { kx[j + sh] = kx[j] + up; kv[j + sh] = kv[j]; }
        for (int j = 0; j < k; ++j) kx[j] -= down;
        kx[k] = ys - down; kv[k] = 0.0;
        kx[k + 1] = ys + up; kv[k + 1] = 0.0;
        const double cp = cap(t), first = kx[0], last = kx[n2 - 1];
        code = (unsigned)br;
        if (first > 0.0) { lo = first; code |= 4u; } else lo = 0.0;
        if (last < cp) { hi = last; code |= 8u; } else hi = cp;
        if (hi < lo) hi = lo;
        int a = 0, b = n2 - 1;
        while (a + 1 < n2 && kx[a + 1] <= lo) ++a;
        while (b > 0 && kx[b - 1] >= hi) --b;
        double vlo = kx[a] == lo ? kv[a] : rb_interp(kx[a], kv[a], kx[a + 1], kv[a + 1], lo);
        double vhi = kx[b] == hi ? kv[b] : rb_interp(kx[b - 1], kv[b - 1], kx[b], kv[b], hi);
        if (!(lo < hi)) { vlo = vhi = 0.0; code |= 16u; }
        sg = rb_fold(sg, code);
        const double ct = c[t] - shift;
        int m = 1;
        for (int j = a + 1; j < b; ++j, ++m) {      // (m <= j: ascending copies overwrite nothing unread)
            const double x = kx[j];
            kv[m] = kv[j] + q * (x - ct);
            kx[m] = x;
        }
        kx[0] = lo; kv[0] = vlo + q * (lo - ct);
        kx[m] = hi; kv[m] = vhi + q * (hi - ct);
        n = m + 1;
    }
    double pn = rb_argmin(kx, kv, n, br);
    sg = rb_fold(sg, (unsigned)br);
    double total = pn;
    if (out) out[T - 1] = pn;
    sg = rb_fold(sg, (pn <= 0.0 ? 1u : 0u) | (pn >= cap(T - 1) ? 2u : 0u));
    for (int t = T - 1; t > 0; --t) {
        const double ys = y[t - 1], a = pn - up, b = pn + down;
        code = 0;
        if (ys < a) { pn = a; code = 4u; }           // the ramp up into t is tight
        else if (ys > b) { pn = b; code = 8u; }      // the ramp down into t is tight
        else pn = ys;
        code |= (pn <= 0.0 ? 1u : 0u) | (pn >= cap(t - 1) ? 2u : 0u);
        sg = rb_fold(sg, code);
        total += pn;
        if (out) out[t - 1] = pn;
    }
    *sum = total;
    *sig = sg;
    return true;
}

// Candidate j of a batch. kind 0: the geometric grid a 2^j (a = +-first); 1: the 64 points a + (b - a) (j + 1) / 65, inside the
// bracket; 2: a itself (a batch of one: the secant point's check)
DOPF_RB_FN double rb_candidate(int kind, double a, double b, int j)
{
    if (kind == 0) return a * (double)(1ull << j);
    if (kind == 1) return a + (b - a) * ((double)(j + 1) * (1.0 / 65.0));
    return a;
}

// The search. It asks one thing of the row, a batch probe:
//     void eval(int kind, double a, double b, int n)    run the programme at the candidates rb_candidate(kind, a, b, j), j < n
//     double phi(int j), unsigned long long sig(int j)  the sum and the signature of candidate j of the last batch
// (on the device a lane holds its candidate's pair and phi / sig are shuffles; a candidate whose programme failed reports phi = NaN).
// phi0 = phi(0); [lo, hi] the budget; first > 0: a lower bound of |nu*| (|phi0 - bound| over the largest slope phi can have, T / q:
// a projection does not expand); tol: how far from the bound a stored row's sum may lie.
// Returns 0: nu = 0 keeps the budget (no batch); 1: *nu is the root — x(*nu) has been evaluated and its sum meets the bound within
// tol, or no double is left between the bracket's ends; -1: max_rounds batches were not enough, or the bound is out of reach
// (*nu = 0: the caller keeps the step at 0). *rounds: batches spent.
// Round 1 brackets on the geometric grid; every later round puts 64 points inside the bracket and keeps the pair of neighbours around
// the crossing. Two neighbours with the same signature end the search at their secant point, once its own sum has met the bound —
// a miss counts as "signatures differ", and the point becomes an end of the bracket.
template <class Batch>
DOPF_RB_FN int ramp_budget_search(Batch &bt, double phi0, double lo, double hi, double first, double tol, int max_rounds, double *nu,
                                  int *rounds)
{
    *nu = 0.0;
    *rounds = 0;
    if (phi0 >= lo && phi0 <= hi) return 0;
    const bool up = phi0 > hi;                  // nu* > 0: the row must come down
    const double target = up ? hi : lo;
    // (a NaN is neither beyond nor a root: the scan stops there and the candidate becomes the far end, with a signature of its own)
    auto beyond = [&](double f) { return up ? f > target + tol : f < target - tol; };
    auto meets = [&](double f) { return f >= target - tol && f <= target + tol; };
    double a = 0.0, fa = phi0, b = 0.0, fb = phi0;
    unsigned long long sa = 0, sb = 0;
    bool known = false, missed = false;         // a's signature is known (nu = 0 has none); the last secant point missed
    int n = 0, kind = 0;
    double ca = up ? first : -first, cb = 0.0;
    for (;;) {
        if (n >= max_rounds) { *rounds = n; return -1; }
        bt.eval(kind, ca, cb, kRampBudgetLanes);
        ++n;
        int j = 0;
        DOPF_RB_NOUNROLL
        while (j < kRampBudgetLanes && beyond(bt.phi(j))) ++j;
        if (j < kRampBudgetLanes && meets(bt.phi(j))) { *nu = rb_candidate(kind, ca, cb, j); *rounds = n; return 1; }
        if (j == kRampBudgetLanes && kind == 0) { *rounds = n; return -1; }        // the bound is out of reach
        const double a0 = a, b0 = b;
        if (j > 0) { a = rb_candidate(kind, ca, cb, j - 1); fa = bt.phi(j - 1); sa = bt.sig(j - 1); known = true; }
        if (j < kRampBudgetLanes) { b = rb_candidate(kind, ca, cb, j); fb = bt.phi(j); sb = bt.sig(j); }
        const bool moved = kind == 0 || a != a0 || b != b0;
        missed = false;
        for (;;) {
            const double mid = a + 0.5 * (b - a);
            const bool room = up ? (mid > a && mid < b) : (mid < a && mid > b);
            if (!room || !moved || !(fb == fb)) { *nu = (fb == fb) ? b : 0.0; *rounds = n; return (fb == fb) ? 1 : -1; }
            if (!(known && sa == sb) || missed) break;
            // the same active set at both ends: x is affine between them
            double sec = fa != fb ? a + (fa - target) * ((b - a) / (fa - fb)) : b;
            sec = up ? rb_min(rb_max(sec, a), b) : rb_max(rb_min(sec, a), b);
            if (n >= max_rounds) { *rounds = n; return -1; }
            bt.eval(2, sec, 0.0, 1);
            ++n;
            const double f = bt.phi(0);
            if (meets(f)) { *nu = sec; *rounds = n; return 1; }
            missed = true;
            if (f == f && sec != a && sec != b) {
                if (beyond(f)) { a = sec; fa = f; sa = bt.sig(0); }
                else { b = sec; fb = f; sb = bt.sig(0); }
            }
        }
        kind = 1; ca = a; cb = b;
    }
}

}  // namespace dopf
