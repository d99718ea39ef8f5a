// budget_root.h — the one-multiplier root search of a generator row under an energy budget (DOPF_F2_GEN_ENERGY_BUDGET).
// Plain C++, no HIP include: gen_budget.h runs it on every lane of the wave that owns the row (all lanes hold the same values: the
// probe's sums are wave reductions), tests/budget_main.cpp as a host program under sanitizers.
//
// With a multiplier nu on the budget row, timestep t's step is x_t(nu): the row's usual step with gen_mc + nu for gen_mc, clipped to
// [0, cap_t]. Every x_t is continuous, piecewise linear and non-increasing in nu, so phi(nu) = sum_t x_t(nu) is too. The row's step
// is x(0) where lo <= phi(0) <= hi, else x(nu*) with phi(nu*) = hi (nu* > 0) or phi(nu*) = lo (nu* < 0).
//
// The search asks one thing of the row, a probe:
//     BudgetProbe probe(double a, double m, double b)
// phi(m), and whether EVERY timestep lies on the same linear piece at m as at a (sameA) and as at b (sameB): the same clip state
// and, where the unclipped step is piecewise linear itself (a network's table), the same interval of it — budget_piece forms such a
// piece number. atLo / atHi: every timestep is clipped at 0 / at its cap at m (nothing is left to move further that way).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_BR_FN __host__ __device__ inline
#else
#define DOPF_BR_FN inline
#endif

namespace dopf {

struct BudgetProbe {
    double phi;
    bool sameA, sameB, atLo, atHi;
};

// evaluations of phi a row may spend (bracket and refinement together) before it gives up: doubling covers a factor 2^60 between
// the first step and the root, and every two refinement steps halve the bracket at least
constexpr int kBudgetMaxEvals = 192;

constexpr int kBudgetFixed = -1;       // the piece of a timestep whose box is one point (cap <= 0): at 0 and at its cap at once

// the linear piece of a timestep whose unclipped step is u, on the interval `interval` (>= 0) of its own pieces
DOPF_BR_FN int budget_piece(double u, double cap, int interval)
{
    if (!(cap > 0.0)) return kBudgetFixed;
    if (u <= 0.0) return 0;
    if (u >= cap) return 1;
    return 2 + interval;
}

// ... of a timestep whose box is [floor, cap] (dopf_set_generator_budget_min_output; floor = fmin(p_min, cap) >= 0): one
// point where !(cap > floor), piece 0 on the floor, piece 1 on the cap. At floor = 0 the three-argument function's values
DOPF_BR_FN int budget_piece(double u, double floor, double cap, int interval)
{
    if (!(cap > floor)) return kBudgetFixed;
    if (u <= floor) return 0;
    if (u >= cap) return 1;
    return 2 + interval;
}

// a running summary of the pieces of a probe (the row's own loop over t feeds it; a wave then reduces the four flags with AND).
// With floors "atLo" reads "every step on its floor" (piece 0 is the box's lower end, whatever it is): nothing changes here
struct BudgetSame {
    bool sameA = true, sameB = true, atLo = true, atHi = true;
    DOPF_BR_FN void add(int pa, int pm, int pb)
    {
        sameA = sameA && pa == pm;
        sameB = sameB && pb == pm;
        atLo = atLo && (pm == 0 || pm == kBudgetFixed);
        atHi = atHi && (pm == 1 || pm == kBudgetFixed);
    }
};

// The search. phi0 = phi(0); [lo, hi] the budget; step > 0: a first distance from 0 (a lower bound of |nu*| makes the best one:
// |phi0 - bound| over the largest slope phi can have). Returns 0: nu = 0 keeps the budget (no probe), 1: *nu is the root — exact
// up to the rounding of one division, since phi is linear between the last bracket's ends — and -1: max_evals probes were not
// enough (*nu = 0: the caller keeps the step at 0). *evals: probes spent.
//
// A probe that meets the bound exactly ends the search: it is a root (e_max = 0 and e_min = sum cap end this way).
// 1. bracket: a = 0, b = +-step, doubled until phi(b) crosses the bound (a follows: phi(a) stays strictly beyond it). A probe at
//    which nothing can move further (atLo going up, atHi going down) ends the search there: the bound is the box's own sum, up to
//    the rounding of that sum. With floors (the four-argument budget_piece) a search going up that ends this way ends on
//    e_max = sum floor, the smallest bound dopf_set_generator_budget_min_output allows: the search itself needs no change.
// 2. refinement: while some timestep changes its piece between a and b, probe a point strictly inside — the midpoint and the secant
//    point in turn — and keep the half that holds the root. The pieces' breakpoints are finitely many and the midpoint steps halve
//    the bracket, so either no breakpoint is left strictly inside (phi is linear on [a, b]: one division) or no double is left
//    between a and b (the same division then picks one of two neighbours; phi is continuous).
template <class Probe>
DOPF_BR_FN int budget_root(Probe &&probe, double phi0, double lo, double hi, double step, int max_evals, double *nu, int *evals)
{
    *nu = 0.0;
    *evals = 0;
    if (phi0 >= lo && phi0 <= hi) return 0;
    const bool up = phi0 > hi;                  // nu* > 0: the row must come down
    const double target = up ? hi : lo;
    double a = 0.0, fa = phi0, b = up ? step : -step, fb = phi0;
    bool same = false;
    int n = 0;
    for (;;) {
        if (n >= max_evals) { *evals = n; return -1; }
        const BudgetProbe r = probe(a, b, b);
        ++n;
        if (r.phi == target) { *nu = b; *evals = n; return 1; }
        if (up ? r.phi < target : r.phi > target) { fb = r.phi; same = r.sameA; break; }
        if (up ? r.atLo : r.atHi) { *nu = b; *evals = n; return 1; }
        a = b; fa = r.phi; b = 2.0 * b;
    }
    for (;;) {
        const double mid = a + 0.5 * (b - a);
        const bool room = up ? (mid > a && mid < b) : (mid < a && mid > b);
        // (fa lies strictly beyond the target and fb at or across it: fa != fb)
        const double sec = fa != fb ? a + (fa - target) * ((b - a) / (fa - fb)) : b;
        if (same || !room) {
            *nu = up ? (sec < a ? a : sec > b ? b : sec) : (sec > a ? a : sec < b ? b : sec);
            *evals = n;
            return 1;
        }
        if (n >= max_evals) { *nu = 0.0; *evals = n; return -1; }
        const bool sec_inside = up ? (sec > a && sec < b) : (sec < a && sec > b);
        const double m = ((n & 1) && sec_inside) ? sec : mid;
        const BudgetProbe r = probe(a, m, b);
        ++n;
        if (r.phi == target) { *nu = m; *evals = n; return 1; }
        if (up ? r.phi > target : r.phi < target) { a = m; fa = r.phi; same = r.sameB; }
        else { b = m; fb = r.phi; same = r.sameA; }
    }
}

}  // namespace dopf
