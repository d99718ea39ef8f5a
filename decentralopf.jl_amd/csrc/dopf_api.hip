// dopf_api.hip — host side of libdopf_hip: the C ABI of include/dopf.h.
//
// One context = one GPU's shard of the agents + a replica of the O((N+L)T) consensus state.
// An ADMM iteration is a short kernel chain on one stream (with DOPF_F_OVERLAP_AGENTS the storage
// kernel is forked onto a side stream so that it overlaps the bandwidth-bound generator kernel):
//   [k_tables] -> k_gen_update -> k_sto_update -> [k_slack] -> k_reduce -> (all-reduce) -> k_dual -> k_price
// dopf_iterate replays it from a captured hipGraph (UNROLL iterations per graph launch) so that the
// loop runs without host round trips; convergence is tested on the device and freezes the state.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "dopf_ctx.h"
#include "trace.h"

using namespace dopf;

namespace {

#ifndef DOPF_UNROLL
#define DOPF_UNROLL 16
#endif
constexpr int kUnroll = DOPF_UNROLL, kMid = 4;
constexpr int kGraphIters[3] = {kUnroll, kMid, 1};      // iterations per launch of dopf_ctx::graphs[*].g, in launch order
constexpr int kCheckEvery = 512;
thread_local char g_create_err[512];

}  // namespace

namespace dopf {

int fail(dopf_ctx *c, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c ? c->err : g_create_err, 512, fmt, ap);
    va_end(ap);
    return code;
}

// a call that owns a temporary context (dopf_central_solve) hands the context's message to dopf_last_error(NULL)
// before the context goes away
void keep_error(const dopf_ctx *c)
{
    if (c && c->err[0]) { strncpy(g_create_err, c->err, 511); g_create_err[511] = 0; }
}


// DOPF_F_STO_TERMINAL_LEVEL: the band [lo, hi] meets the end levels reachable from e0 in T steps of at most pm,
// [max(0, e0 - T pm), min(em, e0 + T pm)]
static bool band_reachable(double e0, double lo, double hi, double pm, double em, int T)
{
    const double span = (double)T * pm;
    return lo <= std::min(em, e0 + span) && hi >= std::max(0.0, e0 - span);
}

// DOPF_F_STO_EFFICIENCY: a step moves the level by at most be pm up and al pm down (al = 1 / eta_d, be = eta_c):
// [max(0, e0 - T al pm), min(em, e0 + T be pm)]
static bool band_reachable(double e0, double lo, double hi, double pm, double em, int T, double al, double be)
{
    return lo <= std::min(em, e0 + (double)T * be * pm) && hi >= std::max(0.0, e0 - (double)T * al * pm);
}

// sorted storage i of the context: the stored band is reachable from e0 (contexts with DOPF_F_STO_EFFICIENCY: under the stored efficiencies)
static bool band_reachable_ctx(const dopf_ctx *c, int i, double e0, double lo, double hi)
{
    if (c->q.flags & DOPF_F_STO_EFFICIENCY)
        return band_reachable(e0, lo, hi, c->sto_pmax_h[i], c->sto_at(kStoEmax, i), c->v.T, c->sto_at(kStoAlpha, i), c->sto_at(kStoBeta, i));
    return band_reachable(e0, lo, hi, c->sto_pmax_h[i], c->sto_at(kStoEmax, i), c->v.T);
}

// every extension's first check: the context was created with the extension's flag (`what_needs`: "line ratings need")
static int needs_flag(dopf_ctx *c, unsigned flag, const char *what_needs, const char *flag_name)
{
    if (c->q.flags & flag) return DOPF_OK;
    return fail(c, DOPF_E_UNSUPPORTED, "%s %s at dopf_create", what_needs, flag_name);
}
#define NEEDS_FLAG(c, what_needs, flag) needs_flag(c, flag, what_needs, #flag)

// dopf_set_storage_initial_level's checks: the flag, and 0 <= e0[s] <= emax[s] for the caller's storage s (no NaN); with
// DOPF_F_STO_TERMINAL_LEVEL also that the stored band stays reachable from e0 (NULL: from 0)
int check_initial_levels(dopf_ctx *c, const double *e0)
{
    if (int rc = NEEDS_FLAG(c, "storage initial levels need", DOPF_F_STO_INITIAL_LEVEL)) return rc;
    const bool band = (c->q.flags & DOPF_F_STO_TERMINAL_LEVEL) != 0;
    if (!e0 && !band) return DOPF_OK;
    for (int i = 0; i < c->v.S; ++i) {
        const int a = c->sto_perm[i];
        const double x = e0 ? e0[a] : 0.0;
        if (!(x >= 0.0 && x <= c->sto_at(kStoEmax, i)))
            return fail(c, DOPF_E_INVALID, "initial level of storage %d is %g, outside [0, max_level = %g]", a, x, c->sto_at(kStoEmax, i));
        if (band && !band_reachable_ctx(c, i, x, c->sto_at(kStoEndLo, i), c->sto_at(kStoEndHi, i)))
            return fail(c, DOPF_E_INVALID, "initial level %g of storage %d leaves its terminal band [%g, %g] unreachable in %d steps of %g",
                        x, a, c->sto_at(kStoEndLo, i), c->sto_at(kStoEndHi, i), c->v.T, c->sto_pmax_h[i]);
    }
    return DOPF_OK;
}

// DOPF_F_GEN_RAMP: an anchored generator must be able to come down under its caps — lo_0 = max(0, p_prev - ramp_down),
// lo_t = max(0, lo_{t-1} - ramp_down) <= cap[g,t] for every t. g: the caller's index (the message's); f: the generator's profile, or null
static int ramp_anchor_fits(dopf_ctx *c, const char *entry, int g, double pm, double down, double prev, const double *f)
{
    if (std::isnan(prev)) return DOPF_OK;
    double lo = prev;
    for (int t = 0; t < c->v.T; ++t) {
        lo = std::max(0.0, lo - down);
        const double cap = f ? pm * f[t] : pm;
        if (lo > cap)
            return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot come down from p_prev = %g under its cap %g at t = %d (ramp_down = %g "
                                           "leaves it at %g or above)", entry, g, prev, cap, t, down, lo);
        if (lo == 0.0) break;
    }
    return DOPF_OK;
}

static int ramp_budget_rows_fit(dopf_ctx *c, const char *entry, bool given_ramp, const double *up, const double *down, const double *prev,
                                bool given_budget, const double *e_min, const double *e_max, bool given_table, const double *profiles,
                                const int32_t *profile_of);

// dopf_set_generator_min_output: a row with a floor needs a path inside floor_t = min(p_min, cap_t) <= P_t <= cap_t under its ramps and
// anchor. The forward intervals F_0 = [max(floor_0, prev - down), min(cap_0, prev + up)] ([floor_0, cap_0] without an anchor),
// F_t = [max(floor_t, lo_{t-1} - down), min(cap_t, hi_{t-1} + up)] hold exactly the values a path can have at t: the row is feasible
// exactly when none is empty (a point of F_{T-1} traces back through them). At p_min = 0 this is ramp_anchor_fits.
// g: the caller's index (the message's); f: the generator's profile, or null; prev: NaN = no anchor
static int ramp_floor_fits(dopf_ctx *c, const char *entry, int g, double pm, double p_min, double up, double down, double prev, const double *f)
{
    double lo = 0.0, hi = 0.0;
    for (int t = 0; t < c->v.T; ++t) {
        const double cap = f ? pm * f[t] : pm, fl = std::min(p_min, cap);
        if (t == 0 && std::isnan(prev)) { lo = fl; hi = cap; }
        else if (t == 0) { lo = std::max(fl, prev - down); hi = std::min(cap, prev + up); }
        else { lo = std::max(fl, lo - down); hi = std::min(cap, hi + up); }
        if (lo > hi)
            return fail(c, DOPF_E_INVALID, "%s: generator g = %d has no path between its floor and its cap under its ramps and anchor at t = %d "
                                           "(at least %g, at most %g; p_min = %g)", entry, g, t, lo, hi, p_min);
    }
    return DOPF_OK;
}

// ... for every row with a floor above 0: the stored floors (gen_min_h), ramps, anchor, profile indices and table, each replaced by the
// caller's where one is given (p_min, up / down / prev: the caller's order; given_ramp says whether the call sets the ramps — a NULL
// then means the default; profiles / profile_of: the availability setter's arguments, with given_table)
static int ramp_floor_rows_fit(dopf_ctx *c, const char *entry, const double *p_min, bool given_ramp, const double *up, const double *down,
                               const double *prev, bool given_table, const double *profiles, const int32_t *profile_of)
{
    if (!c->plan.genRamp || (!p_min && !c->plan.genMinOut)) return DOPF_OK;
    const size_t G = (size_t)c->v.G;
    const int T = c->v.T;
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        const double pmn = p_min ? p_min[a] : c->gen_min_h[i];
        if (!(pmn > 0.0)) continue;
        double u = c->gen_ramp_h[G + i], d = c->gen_ramp_h[2 * G + i], pv = c->gen_ramp_h[3 * G + i];
        if (given_ramp) { u = up ? up[a] : INFINITY; d = down ? down[a] : INFINITY; pv = prev ? prev[a] : std::nan(""); }
        const double *f = nullptr;
        if (given_table) {
            const int k = profile_of ? profile_of[a] : -1;
            if (k >= 0) f = profiles + (size_t)k * T;
        } else {
            const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
            if (k >= 0) f = c->gen_avail_h.data() + (size_t)k * T;
        }
        if (int rc = ramp_floor_fits(c, entry, a, c->gen_ramp_h[i], pmn, u, d, pv, f)) return rc;
    }
    return DOPF_OK;
}

// dopf_set_generator_min_output's checks: the ramp flag, no budget, 0 <= p_min <= gen_pmax (finite), and every row with a floor has a
// path under the stored ramps, anchor and availability table
int check_generator_min_output(dopf_ctx *c, const double *p_min)
{
    if (!(c->q.flags & DOPF_F_GEN_RAMP))
        return fail(c, DOPF_E_UNSUPPORTED, "minimum output runs on the ramp kernels: it needs DOPF_F_GEN_RAMP at dopf_create (on a network "
                                           "DOPF_F_GEN_RAMP_NETWORK too; the ramps stay +inf until they are set)");
    if (c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET)
        return fail(c, DOPF_E_UNSUPPORTED, "minimum output does not combine with DOPF_F2_GEN_ENERGY_BUDGET (nor with the pair, "
                                           "DOPF_F2_GEN_RAMP_BUDGET): floors inside the multiplier search are not built");
    if (!p_min) return DOPF_OK;
    for (int i = 0; i < c->v.G; ++i) {
        const int a = c->gen_perm[i];
        if (!(p_min[a] >= 0.0 && p_min[a] <= c->gen_ramp_h[i]))
            return fail(c, DOPF_E_INVALID, "dopf_set_generator_min_output: p_min[%d] is %g, outside [0, gen_pmax = %g]", a, p_min[a], c->gen_ramp_h[i]);
    }
    return ramp_floor_rows_fit(c, "dopf_set_generator_min_output", p_min, false, nullptr, nullptr, nullptr, false, nullptr, nullptr);
}

// dopf_set_generator_ramp's checks: the flag, both ramp arrays or neither, no NaN, ramps >= 0, p_prev in [0, gen_pmax], and every
// anchored generator able to stay under its caps (the stored availability table)
int check_generator_ramp(dopf_ctx *c, const double *up, const double *down, const double *prev)
{
    if (int rc = NEEDS_FLAG(c, "generator ramp limits need", DOPF_F_GEN_RAMP)) return rc;
    if (int rc = check_generator_ramp_values(c, "dopf_set_generator_ramp", c->gen_ramp_h.data(), c->gen_avail_h.data(), up, down, prev)) return rc;
    // dopf_set_generator_min_output: ... and every row with a stored floor keeps a path under the new ramps and anchor
    if (int rc = ramp_floor_rows_fit(c, "dopf_set_generator_ramp", nullptr, true, up, down, prev, false, nullptr, nullptr)) return rc;
    // DOPF_F2_GEN_RAMP_BUDGET: ... and every row jointly feasible with its stored budget
    return ramp_budget_rows_fit(c, "dopf_set_generator_ramp", true, up, down, prev, false, nullptr, nullptr, false, nullptr, nullptr);
}

// ... without the flag: the values alone, for `entry` (the name the messages carry). pmax: the capacities in sorted order; table:
// the availability profiles [t + T*k] that the context's profile indices (gen_prof_h; none: every generator at its capacity) refer to
int check_generator_ramp_values(dopf_ctx *c, const char *entry, const double *pmax, const double *table, const double *up, const double *down,
                                const double *prev)
{
    if (!up != !down) return fail(c, DOPF_E_INVALID, "%s: ramp_up and ramp_down must both be given or both be NULL", entry);
    const int G = c->v.G, T = c->v.T;
    for (int i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        const double pm = pmax[i];
        if (up) {
            if (std::isnan(up[a]) || up[a] < 0.0) return fail(c, DOPF_E_INVALID, "%s: ramp_up[%d] is %g (>= 0 wanted)", entry, a, up[a]);
            if (std::isnan(down[a]) || down[a] < 0.0) return fail(c, DOPF_E_INVALID, "%s: ramp_down[%d] is %g (>= 0 wanted)", entry, a, down[a]);
        }
        if (!prev) continue;
        if (!(prev[a] >= 0.0 && prev[a] <= pm))
            return fail(c, DOPF_E_INVALID, "%s: p_prev[%d] is %g, outside [0, gen_pmax = %g]", entry, a, prev[a], pm);
        const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
        if (int rc = ramp_anchor_fits(c, entry, a, pm, down ? down[a] : INFINITY, prev[a], k >= 0 ? table + (size_t)k * T : nullptr)) return rc;
    }
    return DOPF_OK;
}

// DOPF_F2_GEN_ENERGY_BUDGET: a generator must be able to deliver its minimum under its caps — e_min <= sum_t cap[g,t], the sum formed
// in t order. g: the caller's index (the message's); f: the generator's profile, or null
static int budget_min_fits(dopf_ctx *c, const char *entry, int g, double pm, double e_min, const double *f)
{
    if (!(e_min > 0.0)) return DOPF_OK;
    double room = 0.0;
    for (int t = 0; t < c->v.T; ++t) room += f ? pm * f[t] : pm;
    if (e_min > room)
        return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot deliver e_min = %g under its caps (sum_t cap[g,t] = %g)", entry, g, e_min, room);
    return DOPF_OK;
}

// DOPF_F2_GEN_RAMP_BUDGET: a row must be feasible under caps, ramps, anchor and budget at once. hi_t: the pointwise-largest path
// (forward hi_0 = min(cap_0, prev + up), hi_t = min(cap_t, hi_{t-1} + up), then backward hi_t = min(hi_t, hi_{t+1} + down)); lo_t: the
// pointwise-smallest (forward with down, backward with up, from 0). The feasible paths form a lattice, so both are feasible where any
// path is, and the row is feasible exactly when lo_t <= hi_t for all t, e_min <= sum hi_t and sum lo_t <= e_max (sums in t order).
// g: the caller's index (the message's); f: the generator's profile, or null; prev: NaN = no anchor
static int ramp_budget_fits(dopf_ctx *c, const char *entry, int g, double pm, double up, double down, double prev, double e_min,
                            double e_max, const double *f)
{
    const int T = c->v.T;
    std::vector<double> hi((size_t)T), lo((size_t)T);
    for (int t = 0; t < T; ++t) {
        const double cap = f ? pm * f[t] : pm;
        if (t == 0) {
            hi[0] = std::isnan(prev) ? cap : std::min(cap, prev + up);
            lo[0] = std::isnan(prev) ? 0.0 : std::max(0.0, prev - down);
        } else {
            hi[(size_t)t] = std::min(cap, hi[(size_t)t - 1] + up);
            lo[(size_t)t] = std::max(0.0, lo[(size_t)t - 1] - down);
        }
    }
    for (int t = T - 2; t >= 0; --t) {
        hi[(size_t)t] = std::min(hi[(size_t)t], hi[(size_t)t + 1] + down);
        lo[(size_t)t] = std::max(lo[(size_t)t], lo[(size_t)t + 1] - up);
    }
    double shi = 0.0, slo = 0.0;
    for (int t = 0; t < T; ++t) {
        if (lo[(size_t)t] > hi[(size_t)t])
            return fail(c, DOPF_E_INVALID, "%s: generator g = %d has no path under its caps, ramps and anchor at t = %d (at least %g, at most %g)",
                        entry, g, t, lo[(size_t)t], hi[(size_t)t]);
        shi += hi[(size_t)t];
        slo += lo[(size_t)t];
    }
    if (e_min > shi)
        return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot deliver e_min = %g under its caps, ramps and anchor (the largest path sums to %g)",
                    entry, g, e_min, shi);
    if (slo > e_max)
        return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot stay under e_max = %g under its ramps and anchor (the smallest path sums to %g)",
                    entry, g, e_max, slo);
    return DOPF_OK;
}

// ... for every row of a context with the bit: the stored ramps (gen_ramp_h), budgets (gen_budget_h), profile indices and table, each
// replaced by the caller's where one is given (up / down / prev, e_min / e_max: the caller's order; given_ramp / given_budget say whether
// the call sets them — a NULL then means the default; profiles / profile_of: the availability setter's arguments, with given_table)
static int ramp_budget_rows_fit(dopf_ctx *c, const char *entry, bool given_ramp, const double *up, const double *down, const double *prev,
                                bool given_budget, const double *e_min, const double *e_max, bool given_table, const double *profiles,
                                const int32_t *profile_of)
{
    if (!c->plan.genRampBudget) return DOPF_OK;
    const size_t G = (size_t)c->v.G;
    const int T = c->v.T;
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        double u = c->gen_ramp_h[G + i], d = c->gen_ramp_h[2 * G + i], pv = c->gen_ramp_h[3 * G + i];
        double lo = c->gen_budget_h[G + i], hi = c->gen_budget_h[2 * G + i];
        if (given_ramp) { u = up ? up[a] : INFINITY; d = down ? down[a] : INFINITY; pv = prev ? prev[a] : std::nan(""); }
        if (given_budget) { lo = e_min ? e_min[a] : 0.0; hi = e_max ? e_max[a] : INFINITY; }
        const double *f = nullptr;
        if (given_table) {
            const int k = profile_of ? profile_of[a] : -1;
            if (k >= 0) f = profiles + (size_t)k * T;
        } else {
            const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
            if (k >= 0) f = c->gen_avail_h.data() + (size_t)k * T;
        }
        if (int rc = ramp_budget_fits(c, entry, a, c->gen_ramp_h[i], u, d, pv, lo, hi, f)) return rc;
    }
    return DOPF_OK;
}

// dopf_set_generator_budget_min_output: a row with a floor must be able to stay under its maximum — the sum of
// floor[g,t] = min(p_min, cap[g,t]) over t0 <= t < t1, formed in t order, is at most e_max. With e_min <= sum cap (budget_min_fits,
// budget_win_min_fits) the test is exact: every step's box is non-empty, so the reachable sums are exactly [sum floor, sum cap].
// g: the caller's index (the message's); j: the window, -1 for the whole horizon; f: the generator's profile, or null
static int budget_floor_fits(dopf_ctx *c, const char *entry, int g, int j, int t0, int t1, double pm, double p_min, double e_max, const double *f)
{
    if (e_max == INFINITY) return DOPF_OK;
    double need = 0.0;
    for (int t = t0; t < t1; ++t) need += std::min(p_min, f ? pm * f[t] : pm);
    if (need <= e_max) return DOPF_OK;
    if (j < 0)
        return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot stay under e_max = %g on its floors (p_min = %g: sum_t min(p_min, cap[g,t]) = %g)",
                    entry, g, e_max, p_min, need);
    return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot stay under e_max = %g in window j = %d (t = %d .. %d) on its floors (p_min = %g: their "
                                   "sum is %g)", entry, g, e_max, j, t0, t1 - 1, p_min, need);
}

// what a caller of budget_floor_rows_fit replaces of the stored values (all in the caller's order; a `given` flag says whether the call
// sets that part — a NULL behind it then means the default)
struct BudgetFloorGiven {
    const double *p_min = nullptr;                                  // the floors (null: the stored ones)
    bool budget = false; const double *e_max = nullptr;             // dopf_set_generator_energy_budget
    bool windows = false; int n_win = 0; const int32_t *win_end = nullptr; const double *win_max = nullptr;   // ..._energy_budget_windows
    bool table = false; const double *profiles = nullptr; const int32_t *profile_of = nullptr;                // dopf_set_generator_availability
};

// ... for every row with a floor above 0, against its whole-horizon e_max and every window's
static int budget_floor_rows_fit(dopf_ctx *c, const char *entry, const BudgetFloorGiven &n)
{
    if (!c->plan.genBudget || c->plan.genRamp || (!n.p_min && !c->plan.genBudgetMinOut)) return DOPF_OK;
    const size_t G = (size_t)c->v.G;
    const int T = c->v.T;
    const int nw = n.windows ? n.n_win : (int)c->gen_bw_end_h.size();
    const int32_t *ends = n.windows ? n.win_end : c->gen_bw_end_h.data();
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        const double pmn = n.p_min ? n.p_min[a] : c->gen_bmin_h[i];
        if (!(pmn > 0.0)) continue;
        const double pm = c->gen_budget_h[i];
        const double *f = nullptr;
        if (n.table) {
            const int k = n.profile_of ? n.profile_of[a] : -1;
            if (k >= 0) f = n.profiles + (size_t)k * T;
        } else {
            const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
            if (k >= 0) f = c->gen_avail_h.data() + (size_t)k * T;
        }
        const double hi = n.budget ? (n.e_max ? n.e_max[a] : INFINITY) : c->gen_budget_h[2 * G + i];
        if (int rc = budget_floor_fits(c, entry, a, -1, 0, T, pm, pmn, hi, f)) return rc;
        for (int j = 0; j < nw; ++j) {
            const double wh = n.windows ? (n.win_max ? n.win_max[(size_t)j + (size_t)nw * a] : INFINITY)
                                        : c->gen_bw_h[G * (size_t)nw + (size_t)j + (size_t)nw * i];
            if (int rc = budget_floor_fits(c, entry, a, j, j > 0 ? ends[j - 1] : 0, ends[j], pm, pmn, wh, f)) return rc;
        }
    }
    return DOPF_OK;
}

// dopf_set_generator_budget_min_output's checks: the budget flag, no ramps, 0 <= p_min <= gen_pmax (finite), and every row with a floor
// able to stay under its stored e_max (whole horizon and per window) under the stored availability table
int check_generator_budget_min_output(dopf_ctx *c, const double *p_min)
{
    const char *entry = "dopf_set_generator_budget_min_output";
    if (!(c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET))
        return fail(c, DOPF_E_UNSUPPORTED, "%s: floors on budget rows need DOPF_F2_GEN_ENERGY_BUDGET at dopf_create_ex (a DOPF_F_GEN_RAMP context "
                                           "has dopf_set_generator_min_output)", entry);
    if (c->q.flags & DOPF_F_GEN_RAMP)
        return fail(c, DOPF_E_UNSUPPORTED, "%s: not on a DOPF_F_GEN_RAMP context (plain ramp contexts have dopf_set_generator_min_output; floors "
                                           "inside the pair's ramp programme, DOPF_F2_GEN_RAMP_BUDGET, are not built)", entry);
    if (!p_min) return DOPF_OK;
    for (int i = 0; i < c->v.G; ++i) {
        const int a = c->gen_perm[i];
        if (!(std::isfinite(p_min[a]) && p_min[a] >= 0.0 && p_min[a] <= c->gen_budget_h[i]))
            return fail(c, DOPF_E_INVALID, "%s: p_min[g = %d] is %g, outside [0, gen_pmax = %g]", entry, a, p_min[a], c->gen_budget_h[i]);
    }
    BudgetFloorGiven n;
    n.p_min = p_min;
    return budget_floor_rows_fit(c, entry, n);
}

// dopf_set_generator_energy_budget_windows: window j's minimum must be deliverable under the window's caps — e_min <= sum of cap[g,t]
// over t0 <= t < t1, formed in t order. g: the caller's index (the message's); f: the generator's profile, or null
static int budget_win_min_fits(dopf_ctx *c, const char *entry, int g, int j, int t0, int t1, double pm, double e_min, const double *f)
{
    if (!(e_min > 0.0)) return DOPF_OK;
    double room = 0.0;
    for (int t = t0; t < t1; ++t) room += f ? pm * f[t] : pm;
    if (e_min > room)
        return fail(c, DOPF_E_INVALID, "%s: generator g = %d cannot deliver e_min = %g in window j = %d (t = %d .. %d) under its caps (their sum is %g)",
                    entry, g, e_min, j, t0, t1 - 1, room);
    return DOPF_OK;
}

// dopf_set_generator_energy_budget_windows' checks, in the order of include/dopf.h; n_win == 0 (remove the table) needs the flag and
// NULL pointers alone
int check_generator_energy_budget_windows(dopf_ctx *c, int32_t n_win, const int32_t *win_end, const double *e_min, const double *e_max)
{
    const char *entry = "dopf_set_generator_energy_budget_windows";
    if (!(c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET))
        return fail(c, DOPF_E_UNSUPPORTED, "%s: budgets per sub-window need DOPF_F2_GEN_ENERGY_BUDGET at dopf_create_ex", entry);
    if (c->plan.genRampBudget)
        return fail(c, DOPF_E_UNSUPPORTED, "%s: not on a DOPF_F2_GEN_RAMP_BUDGET context (ramps couple neighbouring windows, so a row no longer "
                                           "separates into one problem per window)", entry);
    const int G = c->v.G, T = c->v.T;
    if (n_win < 0 || n_win > T) return fail(c, DOPF_E_INVALID, "%s: n_win = %d outside [0, T = %d]", entry, n_win, T);
    if (n_win == 0) {
        if (win_end || e_min || e_max) return fail(c, DOPF_E_INVALID, "%s: n_win = 0 removes the table and takes NULL pointers only", entry);
        return DOPF_OK;
    }
    if (!win_end) return fail(c, DOPF_E_INVALID, "%s: win_end is NULL with n_win = %d", entry, n_win);
    for (int j = 0; j < n_win; ++j)
        if (win_end[j] <= (j > 0 ? win_end[j - 1] : 0))
            return fail(c, DOPF_E_INVALID, "%s: win_end[j = %d] = %d is not above %d (the ends are strictly increasing from above 0)", entry, j, win_end[j],
                        j > 0 ? win_end[j - 1] : 0);
    if (win_end[n_win - 1] != T)
        return fail(c, DOPF_E_INVALID, "%s: the last end win_end[j = %d] = %d is not T = %d", entry, n_win - 1, win_end[n_win - 1], T);
    for (int i = 0; i < G; ++i)
        if (c->gen_budget_h[(size_t)G + i] != 0.0 || c->gen_budget_h[2 * (size_t)G + i] != INFINITY)
            return fail(c, DOPF_E_INVALID, "%s: generator g = %d holds a whole-horizon budget [%g, %g]; call dopf_set_generator_energy_budget(ctx, NULL, NULL) "
                                           "first (one description of the budgets at a time)", entry, c->gen_perm[i], c->gen_budget_h[(size_t)G + i],
                        c->gen_budget_h[2 * (size_t)G + i]);
    for (int i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
        const double *f = k >= 0 ? c->gen_avail_h.data() + (size_t)k * T : nullptr;
        for (int j = 0; j < n_win; ++j) {
            const size_t at = (size_t)j + (size_t)n_win * a;
            const double lo = e_min ? e_min[at] : 0.0, hi = e_max ? e_max[at] : INFINITY;
            if (std::isnan(lo) || std::isinf(lo) || lo < 0.0)
                return fail(c, DOPF_E_INVALID, "%s: e_min of g = %d, j = %d is %g (finite and >= 0 wanted)", entry, a, j, lo);
            if (std::isnan(hi) || hi < 0.0) return fail(c, DOPF_E_INVALID, "%s: e_max of g = %d, j = %d is %g (>= 0 wanted)", entry, a, j, hi);
            if (lo > hi) return fail(c, DOPF_E_INVALID, "%s: e_min = %g exceeds e_max = %g at g = %d, j = %d", entry, lo, hi, a, j);
            if (int rc = budget_win_min_fits(c, entry, a, j, j > 0 ? win_end[j - 1] : 0, win_end[j], c->gen_budget_h[i], lo, f)) return rc;
        }
    }
    // dopf_set_generator_budget_min_output: ... and every row with a stored floor able to stay under each window's new e_max
    BudgetFloorGiven n;
    n.windows = true; n.n_win = n_win; n.win_end = win_end; n.win_max = e_max;
    return budget_floor_rows_fit(c, entry, n);
}

// dopf_set_generator_energy_budget's checks: the flag, no NaN, e_min finite and >= 0, e_max >= 0, e_min <= e_max, and every minimum
// deliverable under the caps (the stored availability table)
int check_generator_energy_budget(dopf_ctx *c, const double *e_min, const double *e_max)
{
    if (!(c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET))
        return fail(c, DOPF_E_UNSUPPORTED, "generator energy budgets need DOPF_F2_GEN_ENERGY_BUDGET at dopf_create_ex");
    if ((e_min || e_max) && !c->gen_bw_end_h.empty())
        return fail(c, DOPF_E_INVALID, "dopf_set_generator_energy_budget: the context holds budgets per sub-window (n_win = %d); remove them with "
                                       "dopf_set_generator_energy_budget_windows(ctx, 0, NULL, NULL, NULL) first (one description of the budgets at a time)",
                    (int)c->gen_bw_end_h.size());
    if (int rc = check_generator_energy_budget_values(c, "dopf_set_generator_energy_budget", c->gen_budget_h.data(), c->gen_avail_h.data(), e_min, e_max))
        return rc;
    // dopf_set_generator_budget_min_output: ... and every row with a stored floor able to stay under its new e_max
    BudgetFloorGiven n;
    n.budget = true; n.e_max = e_max;
    if (int rc = budget_floor_rows_fit(c, "dopf_set_generator_energy_budget", n)) return rc;
    // DOPF_F2_GEN_RAMP_BUDGET: ... and every row jointly feasible with its stored ramps and anchor
    return ramp_budget_rows_fit(c, "dopf_set_generator_energy_budget", false, nullptr, nullptr, nullptr, true, e_min, e_max, false, nullptr, nullptr);
}

// ... without the flag: the values alone, for `entry` (pmax, table: as check_generator_ramp_values)
int check_generator_energy_budget_values(dopf_ctx *c, const char *entry, const double *pmax, const double *table, const double *e_min,
                                         const double *e_max)
{
    const int G = c->v.G, T = c->v.T;
    for (int i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        const double lo = e_min ? e_min[a] : 0.0, hi = e_max ? e_max[a] : INFINITY;
        if (std::isnan(lo) || std::isinf(lo) || lo < 0.0)
            return fail(c, DOPF_E_INVALID, "%s: e_min[%d] is %g (finite and >= 0 wanted)", entry, a, lo);
        if (std::isnan(hi) || hi < 0.0) return fail(c, DOPF_E_INVALID, "%s: e_max[%d] is %g (>= 0 wanted)", entry, a, hi);
        if (lo > hi) return fail(c, DOPF_E_INVALID, "%s: e_min[%d] = %g exceeds e_max[%d] = %g", entry, a, lo, a, hi);
        const int k = c->gen_prof_h.empty() ? -1 : c->gen_prof_h[i];
        if (int rc = budget_min_fits(c, entry, a, pmax[i], lo, k >= 0 ? table + (size_t)k * T : nullptr)) return rc;
    }
    return DOPF_OK;
}

// the form of dopf_set_generator_availability's arguments: the flag, a table of K >= 0 profiles with every value in [0, 1] (no NaN), and
// every index in [-1, K)
static int check_availability_table(dopf_ctx *c, int32_t K, const double *profiles, const int32_t *profile_of)
{
    if (int rc = NEEDS_FLAG(c, "generator availability needs", DOPF_F_GEN_AVAILABILITY)) return rc;
    if (K < 0) return fail(c, DOPF_E_INVALID, "n_profiles = %d < 0", K);
    if (K > 0 && !profiles) return fail(c, DOPF_E_INVALID, "profiles is NULL with n_profiles = %d", K);
    if (K > 0 && !profile_of) return fail(c, DOPF_E_INVALID, "profile_of is NULL with n_profiles = %d", K);
    const int T = c->v.T, G = c->v.G;
    if ((int64_t)K * T > ((int64_t)1 << 40)) return fail(c, DOPF_E_INVALID, "n_profiles = %d: table too large", K);
    for (int64_t i = 0; i < (int64_t)K * T; ++i) {
        const double f = profiles[i];
        if (std::isnan(f)) return fail(c, DOPF_E_INVALID, "profiles[%lld] (profile %lld, t = %lld) is NaN", (long long)i, (long long)(i / T), (long long)(i % T));
        if (!(f >= 0.0 && f <= 1.0))
            return fail(c, DOPF_E_INVALID, "profiles[%lld] (profile %lld, t = %lld) = %g outside [0, 1]", (long long)i, (long long)(i / T), (long long)(i % T), f);
    }
    if (profile_of)
        for (int g = 0; g < G; ++g)
            if (profile_of[g] < -1 || profile_of[g] >= K)
                return fail(c, DOPF_E_INVALID, "profile_of[%d] = %d outside [-1, %d)", g, profile_of[g], K);
    return DOPF_OK;
}

// dopf_set_generator_availability's checks: the table's form, and the stored anchors, minima and pairs under the new table
int check_generator_availability(dopf_ctx *c, int32_t K, const double *profiles, const int32_t *profile_of)
{
    if (int rc = check_availability_table(c, K, profiles, profile_of)) return rc;
    const int T = c->v.T, G = c->v.G;
    if (c->q.flags & DOPF_F_GEN_RAMP)      // the anchors of dopf_set_generator_ramp, under the new table
        for (int i = 0; i < G; ++i) {
            const int a = c->gen_perm[i], k = profile_of ? profile_of[a] : -1;
            if (int rc = ramp_anchor_fits(c, "dopf_set_generator_availability", a, c->gen_ramp_h[i], c->gen_ramp_h[2 * (size_t)G + i],
                                          c->gen_ramp_h[3 * (size_t)G + i], k >= 0 ? profiles + (size_t)k * T : nullptr)) return rc;
        }
    // the floors of dopf_set_generator_min_output, under the new table
    if (int rc = ramp_floor_rows_fit(c, "dopf_set_generator_availability", nullptr, false, nullptr, nullptr, nullptr, true, profiles, profile_of))
        return rc;
    if (c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET)      // the minima of dopf_set_generator_energy_budget, under the new table
        for (int i = 0; i < G; ++i) {
            const int a = c->gen_perm[i], k = profile_of ? profile_of[a] : -1;
            if (int rc = budget_min_fits(c, "dopf_set_generator_availability", a, c->gen_budget_h[i], c->gen_budget_h[(size_t)G + i],
                                         k >= 0 ? profiles + (size_t)k * T : nullptr)) return rc;
        }
    // the minima of dopf_set_generator_energy_budget_windows, window by window under the new table
    const int nw = (int)c->gen_bw_end_h.size();
    for (int i = 0; i < G && nw > 0; ++i) {
        const int a = c->gen_perm[i], k = profile_of ? profile_of[a] : -1;
        for (int j = 0; j < nw; ++j)
            if (int rc = budget_win_min_fits(c, "dopf_set_generator_availability", a, j, j > 0 ? c->gen_bw_end_h[(size_t)j - 1] : 0, c->gen_bw_end_h[(size_t)j],
                                             c->gen_budget_h[i], c->gen_bw_h[(size_t)j + (size_t)nw * i], k >= 0 ? profiles + (size_t)k * T : nullptr))
                return rc;
    }
    // the floors of dopf_set_generator_budget_min_output against the stored maxima, under the new table
    BudgetFloorGiven n;
    n.table = true; n.profiles = profiles; n.profile_of = profile_of;
    if (int rc = budget_floor_rows_fit(c, "dopf_set_generator_availability", n)) return rc;
    // DOPF_F2_GEN_RAMP_BUDGET: the stored ramps and budgets together, under the new table
    return ramp_budget_rows_fit(c, "dopf_set_generator_availability", false, nullptr, nullptr, nullptr, false, nullptr, nullptr, true, profiles,
                                profile_of);
}

// dopf_set_storage_terminal_level's checks: the flag, both arrays or neither, 0 <= lo <= hi <= emax (no NaN), and the band reachable
// from the stored initial level
int check_terminal_levels(dopf_ctx *c, const double *lo, const double *hi)
{
    if (int rc = NEEDS_FLAG(c, "storage terminal levels need", DOPF_F_STO_TERMINAL_LEVEL)) return rc;
    if (!lo && !hi) return DOPF_OK;
    if (!lo || !hi) return fail(c, DOPF_E_INVALID, "storage terminal levels: lo and hi must both be given or both be NULL");
    for (int i = 0; i < c->v.S; ++i) {
        const int a = c->sto_perm[i];
        const double l = lo[a], h = hi[a], em = c->sto_at(kStoEmax, i);
        if (!(l >= 0.0 && h <= em && l <= h))
            return fail(c, DOPF_E_INVALID, "terminal band of storage %d is [%g, %g], not inside [0, max_level = %g] (or empty)", a, l, h, em);
        if (!band_reachable_ctx(c, i, c->sto_at(kStoE0, i), l, h))
            return fail(c, DOPF_E_INVALID, "terminal band [%g, %g] of storage %d is unreachable from its initial level %g in %d steps of %g",
                        l, h, a, c->sto_at(kStoE0, i), c->v.T, c->sto_pmax_h[i]);
    }
    return DOPF_OK;
}

// dopf_set_storage_efficiency's checks: the flag, both arrays or neither, every value in (0, 1] (no NaN); with
// DOPF_F_STO_TERMINAL_LEVEL also that the stored band stays reachable from the stored e0
int check_storage_efficiency(dopf_ctx *c, const double *eta_c, const double *eta_d)
{
    if (int rc = NEEDS_FLAG(c, "storage efficiencies need", DOPF_F_STO_EFFICIENCY)) return rc;
    if (!eta_c && !eta_d) return DOPF_OK;          // (all 1: the widest reachable range, and the stored pair passed under a narrower one or this)
    if (!eta_c || !eta_d) return fail(c, DOPF_E_INVALID, "storage efficiencies: eta_c and eta_d must both be given or both be NULL");
    const bool band = (c->q.flags & DOPF_F_STO_TERMINAL_LEVEL) != 0;
    for (int i = 0; i < c->v.S; ++i) {
        const int a = c->sto_perm[i];
        const double ec = eta_c[a], ed = eta_d[a];
        if (std::isnan(ec) || std::isnan(ed)) return fail(c, DOPF_E_INVALID, "%s[%d] is NaN", std::isnan(ec) ? "eta_c" : "eta_d", a);
        if (!(ec > 0.0 && ec <= 1.0)) return fail(c, DOPF_E_INVALID, "eta_c[%d] = %g outside (0, 1]", a, ec);
        if (!(ed > 0.0 && ed <= 1.0)) return fail(c, DOPF_E_INVALID, "eta_d[%d] = %g outside (0, 1]", a, ed);
        if (band && !band_reachable(c->sto_at(kStoE0, i), c->sto_at(kStoEndLo, i), c->sto_at(kStoEndHi, i), c->sto_pmax_h[i], c->sto_at(kStoEmax, i), c->v.T, 1.0 / ed, ec))
            return fail(c, DOPF_E_INVALID, "efficiencies eta_c[%d] = %g, eta_d[%d] = %g leave the terminal band [%g, %g] of storage %d unreachable "
                        "from its initial level %g in %d steps of %g", a, ec, a, ed, c->sto_at(kStoEndLo, i), c->sto_at(kStoEndHi, i), a, c->sto_at(kStoE0, i), c->v.T,
                        c->sto_pmax_h[i]);
    }
    return DOPF_OK;
}

// dopf_set_line_rating's checks: the flag, every entry finite and >= 0 (NULL: dopf_create's limits in every timestep)
int check_line_rating(dopf_ctx *c, const double *rating)
{
    if (int rc = NEEDS_FLAG(c, "line ratings need", DOPF_F_LINE_RATING)) return rc;
    if (!rating) return DOPF_OK;
    const int L = c->v.L, T = c->v.T;
    for (int t = 0; t < T; ++t)
        for (int l = 0; l < L; ++l) {
            const double r = rating[l + (size_t)L * t];
            if (!std::isfinite(r) || r < 0.0)
                return fail(c, DOPF_E_INVALID, "dopf_set_line_rating: rating of line l = %d at t = %d is %g (finite and >= 0 wanted)", l, t, r);
        }
    return DOPF_OK;
}

// dopf_set_generator_quadratic_cost's checks: the flag, every entry finite and >= 0 (NULL: all 0)
int check_generator_quadratic_cost(dopf_ctx *c, const double *c2)
{
    if (int rc = NEEDS_FLAG(c, "quadratic generator costs need", DOPF_F_GEN_QUADRATIC_COST)) return rc;
    if (!c2) return DOPF_OK;
    for (int g = 0; g < c->v.G; ++g)
        if (!std::isfinite(c2[g]) || c2[g] < 0.0)
            return fail(c, DOPF_E_INVALID, "dopf_set_generator_quadratic_cost: c2[%d] is %g (finite and >= 0 wanted)", g, c2[g]);
    return DOPF_OK;
}
}  // namespace dopf

namespace {

template <class Tp>
int dev_alloc(dopf_ctx *c, Tp **out, size_t n, bool zero = true)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(Tp);
    static const bool guard = getenv("DOPF_GUARD") != nullptr;
    if (guard) {
        // debugging aid: every array ends on a 2 MiB boundary of its own allocation, so that an access past its end leaves
        // the mapping at once (GPU memory fault at an address that names the array: the ranges are printed)
        const size_t two = 2u << 20, b16 = (bytes + 15) & ~(size_t)15, tot = (b16 + two - 1) / two * two;
        HIPCHK(c, hipMalloc(&p, tot));
        c->allocs.push_back(p);
        char *q = (char *)p + (tot - b16);
        static const bool chatty = atoi(getenv("DOPF_GUARD")) > 1;
        if (chatty) fprintf(stderr, "dopf guard: ctx %p alloc #%zu %zu bytes [%p, %p) base %p\n", (void *)c, c->allocs.size(), bytes, (void *)q, (void *)(q + b16), p);
        if (zero) HIPCHK(c, hipMemsetAsync(q, 0, bytes, c->main));
        *out = (Tp *)q;
        return DOPF_OK;
    }
    HIPCHK(c, hipMalloc(&p, bytes));
    c->allocs.push_back(p);
    if (zero) HIPCHK(c, hipMemsetAsync(p, 0, bytes, c->main));
    *out = (Tp *)p;
    return DOPF_OK;
}

template <class Tp>
int dev_upload(dopf_ctx *c, const Tp **out, const std::vector<Tp> &h)
{
    Tp *p = nullptr;
    int rc = dev_alloc(c, &p, h.size(), false);
    if (rc) return rc;
    // blocking copy: the staging vector is usually a temporary that dies when this returns
    if (!h.empty()) HIPCHK(c, hipMemcpy(p, h.data(), h.size() * sizeof(Tp), hipMemcpyHostToDevice));
    *out = p;
    return DOPF_OK;
}

}  // namespace

namespace dopf {

// DOPF_F_GEN_AVAILABILITY: the caps changed — a row summarised as "all at the cap" (gen_state 1) becomes "mixed" (2)
__global__ void k_demote_full_rows(int *state, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < G && state[g] == 1) state[g] = 2;
}

void launch_demote_full_rows(const DevView &v, hipStream_t s)
{
    if (v.G > 0) hipLaunchKernelGGL(k_demote_full_rows, dim3((v.G + 255) / 256), dim3(256), 0, s, v.gen_state, v.G);
}

void drop_graphs(dopf_ctx *c)
{
    for (auto &gs : c->graphs) {
        for (auto &g : gs.g) {
            if (g) hipGraphExecDestroy(g);
            g = nullptr;
        }
        gs.valid = false;
    }
}

// the device memory of the context's trace (the stream is idle, or the caller has synchronised)
void trace_release(dopf_ctx *c)
{
    dopf_ctx::Trace &t = c->trace;
    if (t.ring) hipFree(t.ring);
    if (t.blk) hipFree(t.blk);
    if (t.level) hipFree(t.level);
    t = dopf_ctx::Trace{};
}

int read_status(dopf_ctx *c)
{
    // (every dopf_iterate ends here: on short calls — 20 iterations of 30 us — the read-back is a visible share of the call)
    if (!c->host_pin && hipHostMalloc((void **)&c->host_pin, sizeof(Status), hipHostMallocDefault) != hipSuccess) {
        c->host_pin = nullptr;
        (void)hipGetLastError();
    }
    Status *dst = c->host_pin ? c->host_pin : &c->host_st;
    HIPCHK(c, hipMemcpyAsync(dst, c->v.st, sizeof(Status), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    if (c->host_pin) c->host_st = *c->host_pin;
    if (c->host_st.res_set == 0 || c->host_st.res_set == 1)       // (k_dual_price_t1024 leaves the maxima as bit patterns, see Status)
        for (int k = 0; k < 3; ++k) memcpy(&c->host_st.res[k], &c->host_st.resbits2[c->host_st.res_set][k], sizeof(double));
    return DOPF_OK;
}

}  // namespace dopf

namespace {

// The per-call part of the chain, from the plan, the communicator's state and whether the quiet chain runs (quiet: quiet_allowed
// and no line flagged at the last look). outside: dopf_local_update / dopf_apply_consensus, iterations driven from outside.
struct Step {
    DevView v;                  // the context's view with the per-launch fields: sliceDual, tail, slackInDual, slackGlobal, quiet
    bool like_single;           // the single-GPU chain: no communicator, or a peer exchange inside a kernel of that chain
    const XchgView *xd;         // copper plate + peer exchange: the one-block dual kernel (or the tail block) exchanges the vector
    bool comm_quiet;            // networks on a peer exchange, no line flagged: k_slack's node sums are exchanged, the dual/price
                                // kernel forms the slack sums behind the exchange — no k_reduce (DevView::slackGlobal)
};

Step make_step(const dopf_ctx *c, bool quiet, bool outside = false)
{
    const Plan &p = c->plan;
    const bool single = c->comm == nullptr && !outside;
    const XchgView *x = outside ? nullptr : comm_xchg(c);
    Step st{};
    st.xd = x && ((c->v.L == 0 && p.sliceDual) || c->tail_xchg) ? x : nullptr;
    st.like_single = single || st.xd != nullptr;
    st.comm_quiet = quiet && !st.like_single && x != nullptr && p.commQuiet;
    st.v = c->v;
    DevView &v = st.v;
    v.sliceDual = st.like_single && p.sliceDual;
    v.tail = st.like_single && c->v.tailDev && (c->comm == nullptr || c->tail_xchg) ? c->v.tailDev : nullptr;
    v.slackInDual = (st.like_single || st.comm_quiet) && p.slackDual;
    v.slackGlobal = st.comm_quiet ? 1 : 0;
    v.quiet = single && v.slackInDual && quiet;
    return st;
}

// the quiet chain may run now: the plan allows it and, on a communicator, a peer exchange serves it (not the tail block's)
bool quiet_allowed(const dopf_ctx *c)
{
    return c->comm ? c->plan.commQuiet && comm_xchg(c) != nullptr && !c->tail_xchg : c->plan.quiet;
}

// after a status read: a quiet chain that parked itself (its dual step flagged a line; the iterations behind it were no-ops) is
// released, and *parked says so; otherwise, unless halted, c->quiet records "no line flagged". (That record tests the plan only,
// not the exchange: quiet_allowed tests the exchange when the next chain is picked, and dopf_debug_quiet reports the record.)
int settle_quiet(dopf_ctx *c, bool *parked)
{
    *parked = c->host_st.halt == 2;
    if (*parked) {
        HIPCHK(c, hipMemsetAsync(&c->v.st->halt, 0, sizeof(int), c->main));
        c->host_st.halt = 0;
        c->quiet = false;
        ++c->quiet_parked;
    } else if (!c->host_st.halt) {
        c->quiet = (c->comm ? c->plan.commQuiet : c->plan.quiet) && c->host_st.walk_last == 0;
    }
    return DOPF_OK;
}

// dopf_iterate_timed's events between the stages of an iteration, E_N per iteration
enum { E_T0, E_T1, E_G0, E_G1, E_S0, E_S1, E_K0, E_K1, E_R1, E_D1, E_X0, E_X1, E_N };

void enqueue_local(dopf_ctx *c, const Step &st, const hipEvent_t *ev = nullptr)
{
    const DevView &v = st.v;
    const Plan &p = c->plan;
    auto mark = [&](int k, hipStream_t s) { if (ev) hipEventRecord(ev[k], s); };
    mark(E_T0, c->main);
    launch_tables(v, p, c->main);
    mark(E_T1, c->main);
    const bool fork = v.nGenItems > 0 && v.nStoItems > 0 && (c->q.flags & DOPF_F_OVERLAP_AGENTS);     // (no fused launch then)
    if (fork) {
        hipEventRecord(c->evFork, c->main);
        hipStreamWaitEvent(c->side, c->evFork, 0);
        mark(E_S0, c->side);
        launch_sto_update(v, p, c->side);
        mark(E_S1, c->side);
        hipEventRecord(c->evJoin, c->side);
    }
    mark(E_G0, c->main);
    if (p.fuseAgents) launch_agents_fused(v, p, c->main);
    else if (p.fuseNet) launch_net_agents(v, p, c->main);
    else launch_gen_update(v, p, c->main);
    mark(E_G1, c->main);
    if (fork) {
        hipStreamWaitEvent(c->main, c->evJoin, 0);
    } else {
        mark(E_S0, c->main);
        if (!p.fuseAgents && !p.fuseNet) launch_sto_update(v, p, c->main);
        mark(E_S1, c->main);
    }
    mark(E_K0, c->main);                    // (v.tail: sums, dual step and stop test happened in the launch above)
    if (!v.tail && !v.quiet) launch_slack(v, c->main);
    mark(E_K1, c->main);
    if (!v.tail && !v.slackInDual) launch_reduce(v, p, c->main);
    mark(E_R1, c->main);
}

void enqueue_apply(dopf_ctx *c, const Step &st, const hipEvent_t *ev = nullptr)
{
    if (!st.v.tail) launch_dual(st.v, c->plan, c->main, st.xd);
    if (ev) for (int k : {E_D1, E_X0, E_X1}) hipEventRecord(ev[k], c->main);
}

// k_trace's argument for the context's active trace
TraceView trace_view(const dopf_ctx *c)
{
    const dopf_ctx::Trace &t = c->trace;
    unsigned long long units = 0;
    for (int k = 0; k < kTraceSections; ++k) units += (t.lay.n[k] + 1) / 2;
    return TraceView{c->v.st, t.blk, t.ring, t.capacity, (unsigned long long)t.lay.slot_bytes, units};
}

// one iteration of the chain on the context's stream; a sharded context (dopf_comm_init) puts the all-reduce
// of the consensus buffer between the local sums and the dual step. ev: dopf_iterate_timed's events for this iteration.
int enqueue_iteration(dopf_ctx *c, bool quiet = false, const hipEvent_t *ev = nullptr)
{
    const Step st = make_step(c, quiet);
    enqueue_local(c, st, ev);
    if (st.comm_quiet) launch_xchg(c->v, *comm_xchg(c), c->main, true);
    else if (!st.like_single) { const int rc = comm_enqueue_allreduce(c); if (rc) return rc; }
    enqueue_apply(c, st, ev);
    if (c->trace.active) launch_trace(trace_view(c), c->main);      // dopf_trace_*: the iteration's slot, behind its last kernel
    return DOPF_OK;
}

int build_graph(dopf_ctx *c, int iters, hipGraphExec_t *out, bool quiet = false)
{
    hipGraph_t g = nullptr;
    // (a sharded context captures the RCCL collective with the kernels; thread-local mode keeps the capture
    // from tripping over what other host threads — other GPUs' drivers — do meanwhile)
    HIPCHK(c, hipStreamBeginCapture(c->main, c->comm ? hipStreamCaptureModeThreadLocal : hipStreamCaptureModeRelaxed));
    int rc = DOPF_OK;
    for (int i = 0; i < iters && rc == DOPF_OK; ++i) rc = enqueue_iteration(c, quiet);
    const hipError_t ec = hipStreamEndCapture(c->main, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (ec != hipSuccess) return fail(c, DOPF_E_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(ec));
    hipError_t e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) return fail(c, DOPF_E_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e));
    return DOPF_OK;
}

int build_graphs(dopf_ctx *c, bool quiet)
{
    dopf_ctx::Graphs &gs = c->graphs[quiet];
    for (int k = 0; k < 3; ++k)
        if (const int rc = build_graph(c, kGraphIters[k], &gs.g[k], quiet)) return rc;
    gs.valid = true;
    return DOPF_OK;
}

// a storage sub-problem that hit the root search's iteration cap leaves an unconverged row behind: report it
int check_solver(dopf_ctx *c)
{
    if (c->host_st.tail_timeout)
        return fail(c, DOPF_E_DEVICE, "the block sums of an iteration did not arrive in the launch's tail block in time; the state is not valid");
    if (c->host_st.xchg_timeout)
        return fail(c, DOPF_E_DEVICE, "peer exchange: a rank's part of the consensus sum did not arrive in time; the state is not valid");
    if (c->host_st.solver_fail > c->solver_fail_seen) {
        const unsigned long long n = c->host_st.solver_fail - c->solver_fail_seen;
        c->solver_fail_seen = c->host_st.solver_fail;
        if (c->plan.genRampNet)
            return fail(c, DOPF_E_SOLVER, "%llu sub-problem(s) were left unsolved (%llu since creation): a storage whose root search did not reach "
                                          "its tolerance, or a generator row whose knots exceeded the capacity of DOPF_F_GEN_RAMP_NETWORK (%d)",
                        n, (unsigned long long)c->host_st.solver_fail, ramp_net_knots(c->v.T, c->v.L));
        if (c->plan.genRampBudget)
            return fail(c, DOPF_E_SOLVER, "%llu sub-problem(s) were left unsolved (%llu since creation): a storage whose root search did not reach "
                                          "its tolerance, or a generator row whose multiplier search under ramps and budget spent its %d evaluations "
                                          "or %d rounds", n, (unsigned long long)c->host_st.solver_fail, kBudgetMaxEvals, kRampBudgetMaxRounds);
        if (c->plan.genBudget)
            return fail(c, DOPF_E_SOLVER, "%llu sub-problem(s) were left unsolved (%llu since creation): a storage whose root search did not reach "
                                          "its tolerance, or a generator row whose energy budget's multiplier search spent its %d evaluations",
                        n, (unsigned long long)c->host_st.solver_fail, kBudgetMaxEvals);
        return fail(c, DOPF_E_SOLVER, "%llu storage sub-problem(s) did not reach the root search's tolerance (%llu since creation)",
                    n, (unsigned long long)c->host_st.solver_fail);
    }
    return DOPF_OK;
}

// ---- dopf_create, stage by stage. The stages run in this order and every effect on the device — streams, allocations, copies,
// ---- the first launch — happens in the order written here. A stage returns a code with its message in the context (validate and
// ---- pick_device, which run before there is one: in dopf_last_error(NULL)'s buffer); dopf_create bails in one place.

// the agents' data in the context's sorted order (sort_agents)
struct Sorted {
    std::vector<double> gmc, gpm, smc, spm, sem;
    std::vector<int> gnode, snode;
};

// 1. the arguments' checks that need no device
int validate(const dopf_problem *p, const dopf_params *q)
{
    if (p->N < 1 || p->T < 1 || p->L < 0 || p->G < 0 || p->S < 0)
        return fail(nullptr, DOPF_E_INVALID, "bad sizes N=%d L=%d T=%d G=%d S=%d", p->N, p->L, p->T, p->G, p->S);
    if (!(q->gamma > 0) || !(q->w_prox > 0) || !(q->w_flow > 0))
        return fail(nullptr, DOPF_E_INVALID, "gamma, w_prox, w_flow must be positive");
    if (!p->demand || (p->L > 0 && (!p->ptdf || !p->f_max)) || (p->G > 0 && (!p->gen_mc || !p->gen_pmax || !p->gen_node)) ||
        (p->S > 0 && (!p->sto_mc || !p->sto_pmax || !p->sto_emax || !p->sto_node)))
        return fail(nullptr, DOPF_E_INVALID, "null array in dopf_problem (every array with a positive extent must be given)");
    for (int g = 0; g < p->G; ++g)
        if (p->gen_node[g] < 0 || p->gen_node[g] >= p->N) return fail(nullptr, DOPF_E_INVALID, "gen_node[%d] out of range", g);
    for (int s = 0; s < p->S; ++s)
        if (p->sto_node[s] < 0 || p->sto_node[s] >= p->N) return fail(nullptr, DOPF_E_INVALID, "sto_node[%d] out of range", s);
    if ((int64_t)p->G * p->T > (int64_t)1 << 40) return fail(nullptr, DOPF_E_INVALID, "problem too large");
    Plan probe{};
    if (p->S > 0 && !sto_config_supported(p->T, &probe) && !(q->flags & (DOPF_F_LONG_HORIZON | DOPF_F_DEBUG_LONG_STO)))
        return fail(nullptr, DOPF_E_UNSUPPORTED, "storage kernel supports T <= 512 (got %d); longer horizons need DOPF_F_LONG_HORIZON", p->T);
    if (2 * p->L > 4096 && !(q->flags & (DOPF_F_WIDE_NETWORK | DOPF_F_DEBUG_WIDE_NET)))
        return fail(nullptr, DOPF_E_UNSUPPORTED, "table kernel supports L <= 2048 (got %d); wider networks need DOPF_F_WIDE_NETWORK", p->L);
    if (wide_chain(p->L, q->flags)) {
        // the kernels index the PTDF (l + L*n) and the line state (l + L*t) in 32-bit ints (net_wide.h, k_slack, line_term)
        if ((int64_t)p->L * p->N >= ((int64_t)1 << 31) || (int64_t)p->L * p->T >= ((int64_t)1 << 31) || (int64_t)p->L >= ((int64_t)1 << 29))
            return fail(nullptr, DOPF_E_UNSUPPORTED, "wide chain needs L*N and L*T below 2^31 (L=%d N=%d T=%d)", p->L, p->N, p->T);
    }
    return DOPF_OK;
}

// 2. the device: dopf_params::device, or the calling thread's current one
int pick_device(const dopf_params *q, int *dev)
{
    if (int rc = check_one_runtime(nullptr)) return rc;
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev < 1)
        return fail(nullptr, DOPF_E_DEVICE, "no HIP device (%s); libdopf_hip has no CPU fallback", hipGetErrorString(e0));
    *dev = q->device;
    if (*dev < 0) hipGetDevice(dev);
    if (*dev >= ndev) return fail(nullptr, DOPF_E_INVALID, "device %d of %d", *dev, ndev);
    return DOPF_OK;
}

// ... and, for the wide chain, room on it. That chain keeps the worst-case table layout: tb_beta, tb_psi 2L, tb_slope
// 2L + 1 doubles, psi0 and m per (n,t), and the slack partials part_U / part_K L doubles each per (n,t). Checked before anything
// is allocated or launched.
int wide_tables_fit(dopf_ctx *c, const dopf_problem *p)
{
    if (!wide_chain(p->L, c->q.flags)) return DOPF_OK;
    const unsigned long long nt = (unsigned long long)p->N * p->T, l2 = 2ull * p->L;
    const unsigned long long need = nt * ((3 * l2 + 1) * sizeof(double) + sizeof(double) + sizeof(int)) + 2 * nt * p->L * sizeof(double);
    size_t freeb = 0, totalb = 0;
    HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
    if (need > freeb)
        return fail(c, DOPF_E_NOMEM, "wide chain: the breakpoint tables and slack partials need %llu bytes, the device has %llu free",
                    need, (unsigned long long)freeb);
    return DOPF_OK;
}

// 3. the streams
int create_streams(dopf_ctx *c)
{
    // (Round 3 ran big networks — configs[3] at full size — with the storage solve on a second stream by itself: 145 -> 136 us per
    // iteration. With generators and storages in one launch whose generator blocks work on both column halves at once
    // (k_net_agents) the one-stream form is ahead again, 117.8 vs 124.9 us; DOPF_F_OVERLAP_AGENTS stays for whoever asks.)
    if (c->q.stream) { c->main = (hipStream_t)c->q.stream; c->own_main = false; }
    else { HIPCHK(c, hipStreamCreateWithFlags(&c->main, hipStreamNonBlocking)); c->own_main = true; }
    // the side stream exists only when it is used: HIP maps streams onto a few hardware queues (4 by default), and a
    // process whose streams outnumber them pays barrier packets on every launch (measured: two contexts + PyTorch's
    // own streams made a 118-node iteration 4x slower)
    if (c->q.flags & DOPF_F_OVERLAP_AGENTS) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    }
    return DOPF_OK;
}

// ... and the view's scalars that come straight from the arguments
void set_scalars(DevView &v, const dopf_problem *p, const dopf_params *q)
{
    v.N = p->N; v.L = p->L; v.T = p->T; v.G = p->G; v.S = p->S; v.M2 = 2 * p->L;
    v.gamma = q->gamma; v.w_flow = q->w_flow; v.w_prox = q->w_prox; v.eps = q->eps; v.mask_thr = q->mask_thr;
    v.max_iters = q->max_iters;
    v.rootCap = (q->flags & DOPF_F_DEBUG_ROOT_CAP) ? 2 : 80;
    v.keepDeltas = (q->flags & DOPF_F_KEEP_DELTAS) ? 1 : 0;
    v.debugLeave = (q->flags & DOPF_F_DEBUG_LEAVE) ? 1 : 0;
    const int A = q->n_agents_global > 0 ? q->n_agents_global : p->G + p->S;
    v.invA = A > 0 ? 1.0 / (double)A : 0.0;
    v.nAgents = (double)A;
    const double a0 = v.w_prox + v.gamma;
    v.cp_ia = 1.0 / a0; v.cp_idet = 1.0 / (a0 * a0 - v.gamma * v.gamma); v.cp_s2 = 2.0 / (a0 + v.gamma);
}

// 4. the agents sorted by node (stable): the permutations into the context, sorted copies of their data into so
int sort_agents(dopf_ctx *c, const dopf_problem *p, Sorted &so)
{
    const int G = p->G, S = p->S;
    c->gen_perm.resize(G);
    c->sto_perm.resize(S);
    std::iota(c->gen_perm.begin(), c->gen_perm.end(), 0);
    std::iota(c->sto_perm.begin(), c->sto_perm.end(), 0);
    // generators: by node, then by marginal cost — a settled dispatch parks the cheap ones at pmax and the dear
    // ones at 0, so the rows the generator kernel may skip (and the ones it must stream) become contiguous
    std::stable_sort(c->gen_perm.begin(), c->gen_perm.end(), [&](int a, int b) {
        return p->gen_node[a] != p->gen_node[b] ? p->gen_node[a] < p->gen_node[b] : p->gen_mc[a] < p->gen_mc[b];
    });
    std::stable_sort(c->sto_perm.begin(), c->sto_perm.end(), [&](int a, int b) { return p->sto_node[a] < p->sto_node[b]; });
    so.gmc.resize(G); so.gpm.resize(G); so.gnode.resize(G);
    so.smc.resize(S); so.spm.resize(S); so.sem.resize(S); so.snode.resize(S);
    for (int i = 0; i < G; ++i) { int a = c->gen_perm[i]; so.gmc[i] = p->gen_mc[a]; so.gpm[i] = p->gen_pmax[a]; so.gnode[i] = p->gen_node[a]; }
    for (int i = 0; i < S; ++i) { int a = c->sto_perm[i]; so.smc[i] = p->sto_mc[a]; so.spm[i] = p->sto_pmax[a]; so.sem[i] = p->sto_emax[a]; so.snode[i] = p->sto_node[a]; }
    for (int i = 0; i < G; ++i) if (!(so.gpm[i] >= 0)) return fail(c, DOPF_E_INVALID, "negative generator capacity");
    for (int i = 0; i < S; ++i) if (!(so.spm[i] >= 0) || !(so.sem[i] >= 0)) return fail(c, DOPF_E_INVALID, "negative storage capacity");
    return DOPF_OK;
}

// 5. what plan_chain needs of the problem, and the fixed-point scales of the one-launch iterations from the problem's bounds —
// |sum of net injections| <= sum of pmax (a storage's D - C lies in [-pmax, pmax]), |cost| <= T * sum |mc| pmax (storages: 2 pmax) —
// so that no accumulator can overflow
Shape shape_and_scales(const dopf_problem *p, const Sorted &so, TailView *tv)
{
    const int N = p->N, T = p->T, G = p->G, S = p->S;
    Shape sh{N, p->L, T, G, S, std::vector<int>(N, 0), std::vector<int>(N, 0), -1, -1};
    for (int i = 0; i < G; ++i) ++sh.gen_at[so.gnode[i]];
    for (int i = 0; i < S; ++i) ++sh.sto_at[so.snode[i]];
    long double bi = 1.0L, bc = 1.0L;
    for (int i = 0; i < G; ++i) { bi += so.gpm[i]; bc += (long double)T * std::fabs(so.gmc[i]) * so.gpm[i]; }
    for (int i = 0; i < S; ++i) { bi += so.spm[i]; bc += (long double)T * std::fabs(so.smc[i]) * 2.0 * so.spm[i]; }
    if (std::isfinite((double)bi) && std::isfinite((double)bc)) {
        sh.ki = 52 - (int)std::ceil(std::log2((double)bi));
        sh.kc = 52 - (int)std::ceil(std::log2((double)bc));
    }
    tv->accStride = (T + 1 + 15) / 16 * 16;                   // replicas on 128-byte lines of their own
    tv->scaleInj = std::ldexp(1.0, std::max(0, std::min(sh.ki, 60))); tv->invInj = 1.0 / tv->scaleInj;
    tv->scaleCost = std::ldexp(1.0, std::max(0, std::min(sh.kc, 60))); tv->invCost = 1.0 / tv->scaleCost;
    return sh;
}

// 6. the chain (dopf_plan.h), and what the kernels read of it
int choose_plan(dopf_ctx *c, const Shape &sh)
{
    hipDeviceProp_t prop{};
    const int cus = hipGetDeviceProperties(&prop, c->device) == hipSuccess ? prop.multiProcessorCount : 0;
    const Plan &pl = c->plan = plan_chain(sh, c->q.flags, cus, (unsigned)c->flags2);
    if (pl.refusal) return fail(c, DOPF_E_UNSUPPORTED, "%s (T=%d)", pl.refusal, sh.T);
    DevView &v = c->v;
    v.use_warm = pl.useWarm; v.genSkip = pl.genSkip; v.genBlocks = v.genRows = pl.genBlocks; v.tablesInDual = pl.tablesInDual;
    v.genTT = pl.genTT; v.genR = pl.genR; v.genTT2 = pl.genTT2; v.genR2 = pl.genR2; v.genTT256 = pl.genTT256;
    v.genChunk = sh.N == 1 ? pl.genItem : 0; v.stoChunk = sh.N == 1 ? pl.stoItem : 0;
    return DOPF_OK;
}

// 7. the layout's scalars (make_layout, dopf_plan.h) into the view, and the dynamic LDS they ask for
int set_layout(dopf_ctx *c, const Layout &lo)
{
    DevView &v = c->v;
    v.nGenItems = (int)lo.gen_items.size(); v.nStoItems = (int)lo.sto_items.size();
    v.maxNodeAgents = lo.maxNodeAgents; v.rowsN = lo.rowsN; v.rowsT = lo.rowsT; v.reduceRB = lo.reduceRB;
    v.dualRowsOff = lo.dualRowsOff; v.dualSdOff = lo.dualSdOff; v.dualLdsBytes = lo.dualLdsBytes;
    HIPCHK(c, raise_lds_limits(v, c->plan));
    return DOPF_OK;
}

// a run of device allocations and uploads that stops at the first failure (rc: its code; the message is in the context)
struct DevRun {
    dopf_ctx *c;
    int rc = DOPF_OK;
    template <class Tp> void zeros(Tp **out, size_t n) { if (!rc) rc = dev_alloc(c, out, n); }
    template <class Tp> void raw(Tp **out, size_t n) { if (!rc) rc = dev_alloc(c, out, n, false); }
    template <class Tp> void upload(const Tp **out, const std::vector<Tp> &h) { if (!rc) rc = dev_upload(c, out, h); }
};

// 8. the problem on the device: the network (with the fmax block)
int upload_network(dopf_ctx *c, const dopf_problem *p)
{
    DevView &v = c->v;
    DevRun d{c};
    const int N = p->N, L = p->L, T = p->T;
    d.upload(&v.demand, std::vector<double>(p->demand, p->demand + (size_t)N * T));
    d.upload(&v.ptdf, std::vector<double>(p->ptdf, p->ptdf + (size_t)L * N));
    std::vector<double> pt((size_t)L * N);
    for (int l = 0; l < L; ++l)
        for (int n = 0; n < N; ++n) pt[n + (size_t)N * l] = p->ptdf[l + (size_t)L * n];
    d.upload(&v.ptdfT, pt);
    // DOPF_F_LINE_RATING: every timestep of the table on f_max until the setter; the graphs capture this address once
    const bool rating = (c->q.flags & DOPF_F_LINE_RATING) && L > 0;
    std::vector<double> fm(fmax_doubles(L, T, rating));
    for (size_t at = 0; at < fm.size(); at += (size_t)L) std::copy(p->f_max, p->f_max + L, fm.begin() + at);
    d.upload(&v.fmax, fm);
    v.fmax_ld = rating ? L : 0;
    return d.rc;
}

// 9. the agents (with the gen_mc block and the storage block, each extension's part at its default; the storage block's mirror) ...
int upload_agents(dopf_ctx *c, const Sorted &so)
{
    DevView &v = c->v;
    DevRun d{c};
    const size_t G = (size_t)v.G, S = (size_t)v.S;
    std::vector<double> mc(so.gmc);
    mc.resize(gen_mc_doubles(v.G, c->plan.genQuad), 0.0);
    d.upload(&v.gen_mc, mc);
    if (c->plan.genRampBudget) {
        // DOPF_F2_GEN_RAMP_BUDGET: ramps (+inf), anchor (NaN), budgets (0, +inf) and k_gen_ramp_budget's scratch behind the capacities;
        // the scratch is never read before it is written. Both host mirrors keep the shapes their setters know
        const size_t n = gen_ramp_budget_doubles(v.G, v.T, v.nGenItems);
        size_t freeb = 0, totalb = 0;
        HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
        if (n * sizeof(double) > freeb)
            return fail(c, DOPF_E_NOMEM, "ramp limits with energy budgets: the pair search's candidates (64 x %d doubles per row in flight, %d rows "
                                         "per generator item) need %llu bytes, the device has %llu free", (int)ramp_row_doubles(v.T), kRampWaves,
                        (unsigned long long)(n * sizeof(double)), (unsigned long long)freeb);
        c->gen_ramp_h.assign(so.gpm.begin(), so.gpm.end());
        c->gen_ramp_h.resize(3 * G, INFINITY);
        c->gen_ramp_h.resize(4 * G, std::nan(""));
        c->gen_budget_h.assign(so.gpm.begin(), so.gpm.end());
        c->gen_budget_h.resize(2 * G, 0.0);
        c->gen_budget_h.resize(3 * G, INFINITY);
        double *blk = nullptr;
        d.raw(&blk, n);
        if (d.rc) return d.rc;
        HIPCHK(c, hipMemcpy(blk, c->gen_ramp_h.data(), 4 * G * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(blk + 4 * G, c->gen_budget_h.data() + G, 2 * G * sizeof(double), hipMemcpyHostToDevice));
        v.gen_pmax = blk;
        // the budget prices of dopf_get_generator_budget_price behind the scratch: zeros until the first x-update
        HIPCHK(c, hipMemset(c->gen_budget_price_d(), 0, G * sizeof(double)));
    } else if (c->plan.genRamp) {
        // DOPF_F_GEN_RAMP: the ramps (+inf), the anchor (NaN: none) and k_gen_ramp's scratch behind the capacities; the scratch is
        // sized from the knots' bound and is never read before it is written
        // (networks, DOPF_F_GEN_RAMP_NETWORK: the scratch of k_gen_ramp_net, at every T, with the tables' kinks beside the ramps' knots)
        const size_t n = gen_pmax_doubles(v.G, v.T, v.nGenItems, true, c->plan.genRampNet ? v.L : 0);
        size_t freeb = 0, totalb = 0;
        HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
        if (n * sizeof(double) > freeb)
            return fail(c, DOPF_E_NOMEM, "ramp limits: the knots of the generators' projection (%d per row in flight) need %llu bytes, the "
                                         "device has %llu free", c->plan.genRampNet ? ramp_net_knots(v.T, v.L) : 2 * v.T + 2,
                        (unsigned long long)(n * sizeof(double)), (unsigned long long)freeb);
        c->gen_ramp_h.assign(so.gpm.begin(), so.gpm.end());
        c->gen_ramp_h.resize(3 * G, INFINITY);
        c->gen_ramp_h.resize(4 * G, std::nan(""));
        c->gen_min_h.assign(G, 0.0);
        double *blk = nullptr;
        d.raw(&blk, n);
        if (d.rc) return d.rc;
        HIPCHK(c, hipMemcpy(blk, c->gen_ramp_h.data(), 4 * G * sizeof(double), hipMemcpyHostToDevice));
        v.gen_pmax = blk;
        // the floors of dopf_set_generator_min_output behind the scratch: zeros until then
        HIPCHK(c, hipMemset(const_cast<double *>(gen_min_output(v)), 0, G * sizeof(double)));
    } else if (c->plan.genBudget) {
        // DOPF_F2_GEN_ENERGY_BUDGET: the budgets behind the capacities, e_min (0) | e_max (+inf) until the setter
        c->gen_budget_h.assign(so.gpm.begin(), so.gpm.end());
        c->gen_budget_h.resize(2 * G, 0.0);
        c->gen_budget_h.resize(3 * G, INFINITY);
        // (the device block is the mirror and, behind it, the budget prices of dopf_get_generator_budget_price: zeros until the first x-update)
        std::vector<double> blk(c->gen_budget_h);
        blk.resize(gen_budget_doubles(v.G), 0.0);
        d.upload(&v.gen_pmax, blk);
    } else {
        d.upload(&v.gen_pmax, so.gpm);
    }
    std::vector<double> mp(2 * G);
    for (size_t i = 0; i < G; ++i) { mp[2 * i] = so.gmc[i]; mp[2 * i + 1] = so.gpm[i]; }
    const double *mpd = nullptr;
    d.upload(&mpd, mp);
    v.gen_mp = reinterpret_cast<const double2 *>(mpd);
    d.upload(&v.sto_mc, so.smc); d.upload(&v.sto_pmax, so.spm);
    c->sto_pmax_h = so.spm;
    c->sto_h.resize((size_t)sto_slots(c->plan) * S);
    for (int slot = 0; slot < sto_slots(c->plan); ++slot)
        for (size_t i = 0; i < S; ++i) c->sto_slot_h(slot)[i] = sto_slot_default(slot, so.sem[i]);
    d.upload(&v.sto_emax, c->sto_h);
    return d.rc;
}

// ... then the layout's arrays, with the bounds on an iteration's moves per node and per line
int upload_layout(dopf_ctx *c, const dopf_problem *p, const Sorted &so, const Layout &lo)
{
    DevView &v = c->v;
    DevRun d{c};
    const int N = v.N, L = v.L;
    d.upload(&v.gen_items, lo.gen_items); d.upload(&v.sto_items, lo.sto_items);
    d.upload(&v.node_gen_beg, lo.node_gen_beg); d.upload(&v.node_sto_beg, lo.node_sto_beg);
    // a generator moves by at most pmax per iteration, a storage's net injection D - C by at most 2 pmax
    std::vector<double> win(N, 0.0);
    for (int i = 0; i < v.G; ++i) win[so.gnode[i]] = std::max(win[so.gnode[i]], so.gpm[i]);
    for (int i = 0; i < v.S; ++i) win[so.snode[i]] = std::max(win[so.snode[i]], 2.0 * so.spm[i]);
    for (int n = 0; n < N; ++n) win[n] = win[n] * (1.0 + 1e-9) + 1e-9;
    d.upload(&v.node_win, win);
    // per line: the largest |kap| W_n over the nodes, kap = w2 h / (w2 + gamma) — if the line's slack offset clears it,
    // every agent of every node has that slack active (or inactive) and the sums are a dot product (k_reduce)
    const double w2 = 2.0 * c->q.w_flow, inv = 1.0 / (w2 + c->q.gamma);
    std::vector<double> reach(L, 0.0);
    for (int l = 0; l < L; ++l)
        for (int n = 0; n < N; ++n) reach[l] = std::max(reach[l], std::fabs(w2 * p->ptdf[l + (size_t)L * n] * inv) * win[n]);
    for (int l = 0; l < L; ++l) reach[l] = reach[l] * (1.0 + 1e-9) + 1e-300;      // strictly beyond every node's own reach
    d.upload(&v.line_reach, reach);
    d.upload(&v.node_gitem_beg, lo.node_gitem_beg); d.upload(&v.node_sitem_beg, lo.node_sitem_beg);
    return d.rc;
}

// 10. the state, zeroed (with the gen_state block: the row states, and DOPF_F_GEN_AVAILABILITY's part behind them)
int alloc_state(dopf_ctx *c, const Layout &lo, TailView &tvh)
{
    DevView &v = c->v;
    const Plan &pl = c->plan;
    DevRun d{c};
    const int N = v.N, L = v.L, T = v.T, G = v.G, S = v.S;
    const size_t NT = (size_t)N * T, LT = (size_t)L * T;
    d.zeros(&v.P, (size_t)G * T);
    d.zeros(&v.gen_state, gen_state_ints(G, pl.genAvail));            // zero = "all zero", which is what P is now
    if (pl.genAvail && !d.rc) {
        // every generator on gen_pmax until the setter (gen_prof(v)); no table yet (its address, gen_avail_slot(v), is null)
        c->gen_prof_h.assign(G, -1);
        HIPCHK(c, hipMemcpyAsync(gen_prof(v), c->gen_prof_h.data(), sizeof(int) * G, hipMemcpyHostToDevice, c->main));
    }
    d.zeros(&v.D, (size_t)S * T); d.zeros(&v.C, (size_t)S * T); d.zeros(&v.E, (size_t)S * T);
    if (L > 0) { d.zeros(&v.dltG, (size_t)G * T); d.zeros(&v.dltS, (size_t)S * T); }
    d.zeros(&v.lam, T); d.zeros(&v.mu, LT); d.zeros(&v.rho, LT);
    d.zeros(&v.lam_used, T); d.zeros(&v.mu_used, LT); d.zeros(&v.rho_used, LT);
    d.zeros(&v.inj, NT); d.zeros(&v.s, T); d.zeros(&v.flow, LT);
    d.zeros(&v.avgU, LT); d.zeros(&v.avgK, LT); d.zeros(&v.price, NT);
    d.zeros(&v.s_used, T); d.zeros(&v.flow_used, LT); d.zeros(&v.avgU_used, LT); d.zeros(&v.avgK_used, LT);
    if (L > 0) {
        d.zeros(&v.tb_beta, NT * v.M2); d.zeros(&v.tb_psi, NT * v.M2);
        d.zeros(&v.tb_slope, NT * (v.M2 + 1)); d.zeros(&v.tb_psi0, NT);
        d.zeros(&v.tb_m, NT);
        d.zeros(&v.part_U, NT * L); d.zeros(&v.part_K, NT * L); d.zeros(&v.node_dsum, NT);
        d.zeros(&v.walk_flag, LT); d.zeros(&v.walk_any, T); d.zeros(&v.tab_skip, T);
    }
    d.zeros(&v.part_ginj, (size_t)v.nGenItems * T); d.zeros(&v.part_gcost, v.nGenItems);
    d.zeros(&v.part_sinj, (size_t)v.nStoItems * T); d.zeros(&v.part_scost, v.nStoItems);
    d.zeros(&v.part_sinj_w, (size_t)v.nStoItems * T); d.zeros(&v.part_scost_w, v.nStoItems);
    if (L > 0) { d.upload(&v.row_of_pos, lo.row_of_pos); d.upload(&v.pos_of_row, lo.pos_of_row); }
    if (L > 0) d.zeros(&v.part_T, (size_t)v.rowsT * T);      // (networks: the ADMM kernels' layout; the rows above serve dopf_central_solve)
    if (L > 0) d.zeros(&v.prev_node, NT);
    d.zeros(&v.nu_prev, (size_t)S * T); d.zeros(&v.nu_valid, S); d.zeros(&v.sto_fail, S);
    d.zeros(&v.item_fail, v.nStoItems);
    d.zeros(&v.part2, (size_t)N * v.reduceRB * T); d.zeros(&v.part2_cost, v.reduceRB);
    d.zeros(&v.reduce_ticket, (size_t)N * ((T + 31) / 32));
    d.zeros(&v.dual_ticket, 1);
    if (pl.tail) {
        d.zeros(&tvh.acc, (size_t)2 * kAccRep * tvh.accStride);
        tvh.expect = agent_blocks(v);
        TailView *tvd = nullptr;
        d.raw(&tvd, 1);
        if (d.rc) return d.rc;
        HIPCHK(c, hipMemcpy(tvd, &tvh, sizeof tvh, hipMemcpyHostToDevice));
        v.tailDev = tvd;
    }
    if (pl.wideNet) {
        std::vector<double> na(N);
        for (int n = 0; n < N; ++n)
            na[n] = (double)((lo.node_gen_beg[n + 1] - lo.node_gen_beg[n]) + (lo.node_sto_beg[n + 1] - lo.node_sto_beg[n]));
        d.upload(&v.node_na, na);
    }
    double *cons = nullptr;
    d.zeros(&cons, NT + 2 * LT + 1);
    c->own_cons = cons;
    v.cons = cons;
    d.zeros(&v.st, 1);
    return d.rc;
}

// 11. the "no result yet" state — zeros everywhere, injection = -demand (helpers/results.jl:14-73) — and the view itself in device
// memory (non-inlined device functions take a pointer to it)
int first_state(dopf_ctx *c)
{
    DevView &v = c->v;
    Status st0{};
    st0.iteration = 1;                                      // admm.jl:29
    st0.res_set = -1;
    HIPCHK(c, hipMemcpyAsync(v.st, &st0, sizeof st0, hipMemcpyHostToDevice, c->main));
    launch_derive(v, c->plan, c->main, false);     // all-zero primal state: the consensus buffer is already zero
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->main));
    c->host_st = st0;
    DevView *dv = nullptr;
    if (const int rc = dev_alloc(c, &dv, 1, false)) return rc;
    v.self = dv;
    HIPCHK(c, hipMemcpy(dv, &v, sizeof(DevView), hipMemcpyHostToDevice));
    return DOPF_OK;
}

// stages 3 to 11 on the context's device
int build_context(dopf_ctx *c, const dopf_problem *p)
{
    if (const int rc = wide_tables_fit(c, p)) return rc;
    if (const int rc = create_streams(c)) return rc;
    set_scalars(c->v, p, &c->q);
    Sorted so;
    if (const int rc = sort_agents(c, p, so)) return rc;
    TailView tvh{};
    const Shape sh = shape_and_scales(p, so, &tvh);
    if (const int rc = choose_plan(c, sh)) return rc;
    const Layout lo = make_layout(sh, c->plan);
    if (const int rc = set_layout(c, lo)) return rc;
    if (const int rc = upload_network(c, p)) return rc;
    if (const int rc = upload_agents(c, so)) return rc;
    if (const int rc = upload_layout(c, p, so, lo)) return rc;
    if (const int rc = alloc_state(c, lo, tvh)) return rc;
    return first_state(c);
}

}  // namespace

extern "C" {

const char *dopf_version(void) { return "libdopf_hip 0.1 (gfx950)"; }

void dopf_default_params(dopf_params *q)
{
    if (!q) return;
    memset(q, 0, sizeof *q);
    q->gamma = 0.3; q->w_flow = 10.0; q->w_prox = 1.0; q->eps = 1e-3; q->mask_thr = 1e-2;
    q->device = -1;
}

const char *dopf_last_error(const dopf_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

int dopf_create(dopf_ctx **out, const dopf_problem *p, const dopf_params *q) { return dopf_create_ex(out, p, q, 0); }

int dopf_create_ex(dopf_ctx **out, const dopf_problem *p, const dopf_params *q, int32_t flags2)
{
    if (!out || !p || !q) return fail(nullptr, DOPF_E_INVALID, "null argument");
    *out = nullptr;
    if (const uint32_t unknown = (uint32_t)flags2 & ~(uint32_t)(DOPF_F2_GEN_ENERGY_BUDGET | DOPF_F2_GEN_RAMP_BUDGET))
        return fail(nullptr, DOPF_E_INVALID, "dopf_create_ex: flags2 has the unknown bit %u (the second word knows DOPF_F2_GEN_ENERGY_BUDGET = 1 "
                                             "and DOPF_F2_GEN_RAMP_BUDGET = 8)", unknown & (~unknown + 1u));
    if (int rc = validate(p, q)) return rc;
    int dev = 0;
    if (int rc = pick_device(q, &dev)) return rc;
    dopf_ctx *c = new (std::nothrow) dopf_ctx;
    if (!c) return fail(nullptr, DOPF_E_NOMEM, "out of host memory");
    c->device = dev;
    c->q = *q;
    c->flags2 = flags2;
    DeviceGuard guard(dev);
    if (const int rc = build_context(c, p)) {
        keep_error(c);
        dopf_destroy(c);
        return rc;
    }
    *out = c;
    return DOPF_OK;
}

void dopf_destroy(dopf_ctx *c)
{
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->main) hipStreamSynchronize(c->main);
    if (c->side) hipStreamSynchronize(c->side);
    drop_graphs(c);
    comm_release(c);
    trace_release(c);
    for (void *p : c->allocs) hipFree(p);
    if (c->evFork) hipEventDestroy(c->evFork);
    if (c->evJoin) hipEventDestroy(c->evJoin);
    if (c->host_pin) hipHostFree(c->host_pin);
    if (c->evT0) hipEventDestroy(c->evT0);
    if (c->evT1) hipEventDestroy(c->evT1);
    if (c->side) hipStreamDestroy(c->side);
    if (c->own_main && c->main) hipStreamDestroy(c->main);
    delete c;
}

int dopf_iterate(dopf_ctx *c, int32_t n_iters, int32_t *iters_done, int32_t *converged)
{
    if (!c || n_iters < 0) return fail(c, DOPF_E_INVALID, "bad argument");
    DeviceGuard guard(c->device);
    const int before = c->host_st.iters_total;
    // with a communicator of more than one rank the chain is launched eagerly unless the caller opts into capturing
    // the collective (DOPF_F_COMM_GRAPH): either way nothing synchronises with the host inside the loop, and the
    // host enqueues an iteration's four launches faster than the GPU retires them
    bool eager = (c->q.flags & DOPF_F_NO_GRAPH) != 0 || (!comm_capturable(c) && !(c->q.flags & DOPF_F_COMM_GRAPH));
    if (!eager && !c->graphs[0].valid) {
        if (const int rc = build_graphs(c, false)) {
            if (!c->comm) return rc;
            // the collective refused to be captured: launch the same chain eagerly from now on (no host sync either way)
            drop_graphs(c);
            (void)hipGetLastError();
            c->q.flags |= DOPF_F_NO_GRAPH;
            eager = true;
        }
    }
    // Enqueue in slices and look at the device status word between slices, so that a converged (or capped)
    // run stops being fed no-op launches; one sync per kCheckEvery iterations costs nothing measurable.
    // DOPF_F_TIME_CALLS (measurement): an event in front of the call's first launch and one behind its last — the device-side
    // span of the call's iterations, without the host's launch latency in front and the status read-back behind
    const bool timed = (c->q.flags & DOPF_F_TIME_CALLS) != 0 && n_iters > 0;
    if (timed) {
        if (!c->evT0) { HIPCHK(c, hipEventCreate(&c->evT0)); HIPCHK(c, hipEventCreate(&c->evT1)); }
        HIPCHK(c, hipEventRecord(c->evT0, c->main));
    }
    int left = n_iters;
    while (left > 0) {
        int slice = std::min(left, kCheckEvery);
        left -= slice;
        // the quiet chain (networks, no line flagged at the last look: no k_slack launch) has graphs of its own, built when first used
        // (on a peer exchange: the chain without k_reduce, see enqueue_iteration — every rank takes the same decision from the same
        // replicated status word at the same iteration)
        const bool quiet = c->quiet && quiet_allowed(c);
        if (quiet && !eager && !c->graphs[1].valid) {
            if (const int rc = build_graphs(c, true)) return rc;
        }
        const int asked = slice, total_before = c->host_st.iters_total;
        if (eager) {
            for (int i = 0; i < slice; ++i) { const int rc = enqueue_iteration(c, quiet); if (rc) return rc; }
        } else {
            const dopf_ctx::Graphs &gs = c->graphs[quiet];
            for (int k = 0; k < 3; ++k)
                for (; slice >= kGraphIters[k]; slice -= kGraphIters[k]) HIPCHK(c, hipGraphLaunch(gs.g[k], c->main));
        }
        HIPCHK(c, hipGetLastError());
        if (timed && left == 0) HIPCHK(c, hipEventRecord(c->evT1, c->main));
        const int rc = read_status(c);
        if (rc) return rc;
        bool parked = false;
        if (const int rc2 = settle_quiet(c, &parked)) return rc2;
        // parked: back to the chain with k_slack, and what is left of the slice is fed again
        if (parked) { left += asked - (c->host_st.iters_total - total_before); continue; }
        if (c->host_st.halt) break;
    }
    c->last_call_ms = -1.0;
    if (timed && left == 0) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->evT0, c->evT1) == hipSuccess) c->last_call_ms = (double)ms;
    }
    if (n_iters == 0) { const int rc = read_status(c); if (rc) return rc; }
    if (iters_done) *iters_done = c->host_st.iters_total - before;
    if (converged) *converged = c->host_st.converged;
    return check_solver(c);
}

double dopf_last_call_ms(const dopf_ctx *c) { return c ? c->last_call_ms : -1.0; }

int dopf_iterate_timed(dopf_ctx *c, int32_t n_iters, dopf_timing *out)
{
    if (!c || !out || n_iters < 1 || n_iters > 4096) return fail(c, DOPF_E_INVALID, "bad argument");
    DeviceGuard guard(c->device);
    if (c->comm) return fail(c, DOPF_E_INVALID, "dopf_iterate_timed drives the single-GPU chain: not on a context joined to a communicator");
    if (c->trace.active) return fail(c, DOPF_E_INVALID, "dopf_iterate_timed: not while a trace is active (dopf_iterate alone advances a traced context)");
    const bool quiet = c->quiet && quiet_allowed(c);          // (the chain dopf_iterate would launch now)
    struct Events {                                     // destroyed on every way out
        std::vector<hipEvent_t> v;
        ~Events() { for (auto e : v) if (e) hipEventDestroy(e); }
    } evs;
    evs.v.assign((size_t)n_iters * E_N, nullptr);
    std::vector<hipEvent_t> &ev = evs.v;
    for (auto &e : ev) HIPCHK(c, hipEventCreate(&e));
    for (int i = 0; i < n_iters; ++i) (void)enqueue_iteration(c, quiet, &ev[(size_t)i * E_N]);     // (no communicator: nothing to fail)
    HIPCHK(c, hipGetLastError());
    int rc = read_status(c);
    if (rc) return rc;
    bool parked = false;
    if ((rc = settle_quiet(c, &parked))) return rc;
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
    memset(out, 0, sizeof *out);
    auto ms = [&](hipEvent_t a, hipEvent_t b) { float f = 0.f; hipEventElapsedTime(&f, a, b); return (double)f; };
    for (int i = 0; i < n_iters; ++i) {
        hipEvent_t *e = &ev[(size_t)i * E_N];
        out->tables_ms += ms(e[E_T0], e[E_T1]);
        out->gen_ms += ms(e[E_G0], e[E_G1]);
        out->sto_ms += ms(e[E_S0], e[E_S1]);
        out->slack_ms += ms(e[E_K0], e[E_K1]);
        out->reduce_ms += ms(e[E_K1], e[E_R1]);
        out->dual_ms += ms(e[E_R1], e[E_D1]);
        out->iter_ms += ms(e[E_T0], e[E_D1]);
        out->empty_ms += ms(e[E_X0], e[E_X1]);
    }
    const double inv = 1.0 / n_iters;
    out->tables_ms *= inv; out->gen_ms *= inv; out->sto_ms *= inv; out->slack_ms *= inv;
    out->reduce_ms *= inv; out->dual_ms *= inv; out->iter_ms *= inv; out->empty_ms *= inv;
    const Plan &p = c->plan;
    const Step st = make_step(c, quiet);
    const DevView &v = st.v;
    out->iters = n_iters;
    out->agents_fused = p.fuseAgents || p.fuseNet;
    out->tail_fused = v.tail ? 1 : 0;
    out->slack_in_dual = (!v.tail && v.slackInDual) ? 1 : 0;
    out->quiet = v.quiet ? 1 : 0;
    out->sto_lean = (p.stoLean && v.S > 0 && v.use_warm) ? 1 : 0;
    out->sto_long = (p.stoLong && v.S > 0) ? 1 : 0;
    return DOPF_OK;
}

int dopf_local_update(dopf_ctx *c)
{
    if (!c) return DOPF_E_INVALID;
    if (c->trace.active) return fail(c, DOPF_E_INVALID, "dopf_local_update: not while a trace is active (dopf_iterate alone advances a traced context)");
    DeviceGuard guard(c->device);
    c->quiet = false;                      // (iterations driven from outside: the next dopf_iterate looks at the flags before it trusts them)
    enqueue_local(c, make_step(c, false, true));
    HIPCHK(c, hipGetLastError());
    return DOPF_OK;
}

int dopf_apply_consensus(dopf_ctx *c)
{
    if (!c) return DOPF_E_INVALID;
    if (c->trace.active) return fail(c, DOPF_E_INVALID, "dopf_apply_consensus: not while a trace is active (dopf_iterate alone advances a traced context)");
    DeviceGuard guard(c->device);
    c->quiet = false;
    enqueue_apply(c, make_step(c, false, true));
    HIPCHK(c, hipGetLastError());
    return DOPF_OK;
}

int64_t dopf_consensus_size(const dopf_ctx *c)
{
    return c ? (int64_t)c->v.N * c->v.T + 2 * (int64_t)c->v.L * c->v.T + 1 : 0;
}

void *dopf_consensus_ptr(dopf_ctx *c) { return c ? (void *)c->v.cons : nullptr; }

int dopf_bind_consensus(dopf_ctx *c, void *device_ptr)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    HIPCHK(c, hipStreamSynchronize(c->main));
    c->v.cons = device_ptr ? (double *)device_ptr : (double *)c->own_cons;
    HIPCHK(c, hipMemcpy(const_cast<DevView *>(c->v.self), &c->v, sizeof(DevView), hipMemcpyHostToDevice));
    drop_graphs(c);
    return DOPF_OK;
}

int dopf_sync(dopf_ctx *c, int32_t *iteration, int32_t *converged)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    int rc = read_status(c);
    if (rc) return rc;
    if (iteration) *iteration = c->host_st.iteration;
    if (converged) *converged = c->host_st.converged;
    return check_solver(c);
}

static int copy_out(dopf_ctx *c, double *dst, const double *src, size_t n)
{
    if (!dst || n == 0) return DOPF_OK;
    HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, c->main));
    return DOPF_OK;
}

int dopf_get_duals(dopf_ctx *c, double *lambda, double *mu, double *rho)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    const size_t LT = (size_t)c->v.L * c->v.T;
    int rc;
    if ((rc = copy_out(c, lambda, c->v.lam, c->v.T))) return rc;
    if ((rc = copy_out(c, mu, c->v.mu, LT))) return rc;
    if ((rc = copy_out(c, rho, c->v.rho, LT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main));
    return DOPF_OK;
}

int dopf_get_duals_used(dopf_ctx *c, double *lambda, double *mu, double *rho)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    const size_t LT = (size_t)c->v.L * c->v.T;
    int rc;
    if ((rc = copy_out(c, lambda, c->v.lam_used, c->v.T))) return rc;
    if ((rc = copy_out(c, mu, c->v.mu_used, LT))) return rc;
    if ((rc = copy_out(c, rho, c->v.rho_used, LT))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main));
    return DOPF_OK;
}

// device rows are in node-sorted order; hand them back in the caller's agent order
static int get_rows(dopf_ctx *c, double *dst, const double *src, const std::vector<int> &perm)
{
    if (!dst || perm.empty()) return DOPF_OK;
    const int T = c->v.T;
    std::vector<double> tmp((size_t)perm.size() * T);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    for (size_t i = 0; i < perm.size(); ++i) memcpy(dst + (size_t)perm[i] * T, tmp.data() + i * T, sizeof(double) * T);
    return DOPF_OK;
}

static int set_rows(dopf_ctx *c, double *dst, const double *src, const std::vector<int> &perm)
{
    if (!src || perm.empty()) return DOPF_OK;
    const int T = c->v.T;
    std::vector<double> tmp((size_t)perm.size() * T);
    for (size_t i = 0; i < perm.size(); ++i) memcpy(tmp.data() + i * T, src + (size_t)perm[i] * T, sizeof(double) * T);
    HIPCHK(c, hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    return DOPF_OK;
}

int dopf_get_primal(dopf_ctx *c, double *P, double *D, double *C, double *E)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = get_rows(c, P, c->v.P, c->gen_perm))) return rc;
    if ((rc = get_rows(c, D, c->v.D, c->sto_perm))) return rc;
    if ((rc = get_rows(c, C, c->v.C, c->sto_perm))) return rc;
    if (E && c->level_from_primal) {         // the level is rebuilt from D and C (the iteration's kernels do not store it)
        launch_derive_level(c->v, c->plan, c->main);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->main));
    }
    if ((rc = get_rows(c, E, c->v.E, c->sto_perm))) return rc;
    return DOPF_OK;
}

int dopf_get_consensus(dopf_ctx *c, double *injection, double *avg_U, double *avg_K, double *line_util, double *total_cost)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    const size_t NT = (size_t)c->v.N * c->v.T, LT = (size_t)c->v.L * c->v.T;
    int rc;
    if ((rc = copy_out(c, injection, c->v.inj, NT))) return rc;
    if ((rc = copy_out(c, avg_U, c->v.avgU, LT))) return rc;
    if ((rc = copy_out(c, avg_K, c->v.avgK, LT))) return rc;
    if ((rc = copy_out(c, line_util, c->v.flow, LT))) return rc;
    if ((rc = read_status(c))) return rc;
    if (total_cost) *total_cost = c->host_st.total_cost;
    return DOPF_OK;
}

int dopf_get_residuals(dopf_ctx *c, double *a, double *b, double *r, int32_t *iteration)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    int rc = read_status(c);
    if (rc) return rc;
    if (a) *a = c->host_st.res[0];
    if (b) *b = c->host_st.res[1];
    if (r) *r = c->host_st.res[2];
    if (iteration) *iteration = c->host_st.iteration;
    return DOPF_OK;
}

int dopf_get_nodal_price(dopf_ctx *c, int32_t which, double *out)
{
    if (!c || !out) return DOPF_E_INVALID;
    const int N = c->v.N, L = c->v.L, T = c->v.T;
    std::vector<double> lam(T), mu((size_t)L * T), rho((size_t)L * T), ptdf((size_t)L * N);
    int rc = which ? dopf_get_duals(c, lam.data(), mu.data(), rho.data())
                   : dopf_get_duals_used(c, lam.data(), mu.data(), rho.data());
    if (rc) return rc;
    DeviceGuard guard(c->device);
    if (L > 0) HIPCHK(c, hipMemcpy(ptdf.data(), c->v.ptdf, ptdf.size() * sizeof(double), hipMemcpyDeviceToHost));
    // lambda_t + sum_l (mu + rho)[l,t] * ptdf[l,n]   (helpers/network_elements.jl:16-25)
    for (int t = 0; t < T; ++t)
        for (int n = 0; n < N; ++n) {
            double p = lam[t];
            for (int l = 0; l < L; ++l) p += (mu[l + (size_t)L * t] + rho[l + (size_t)L * t]) * ptdf[l + (size_t)L * n];
            out[n + (size_t)N * t] = p;
        }
    return DOPF_OK;
}

// scratch of the getters that reduce on the device: allocated once (an allocation per call would be a device-wide
// synchronisation per Result in a record-everything loop), freed with the context's other arrays
static int getter_scratch(dopf_ctx *c, double **out)
{
    if (!c->getter_scratch) {
        int rc = dev_alloc(c, &c->getter_scratch, 3 * (size_t)c->v.N * c->v.T, false);
        if (rc) return rc;
    }
    *out = c->getter_scratch;
    return DOPF_OK;
}

int dopf_get_node_results(dopf_ctx *c, double *generation, double *discharge, double *charge)
{
    if (!c) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    const size_t NT = (size_t)c->v.N * c->v.T;
    double *tmp = nullptr;
    int rc = getter_scratch(c, &tmp);
    if (rc) return rc;
    launch_node_results(c->v, tmp, tmp + NT, tmp + 2 * NT, c->main);
    HIPCHK(c, hipGetLastError());
    double *outs[3] = {generation, discharge, charge};
    for (int k = 0; k < 3; ++k)
        if (outs[k]) HIPCHK(c, hipMemcpyAsync(outs[k], tmp + k * NT, NT * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    return DOPF_OK;
}

// Result.penalty_term (src/structures/results.jl:66-70): the agents' three penalty vectors summed, one device pass
int dopf_get_penalty_sums(dopf_ctx *c, double *penalty)
{
    if (!c || !penalty) return DOPF_E_INVALID;
    const DevView &v = c->v;
    if (v.L == 0 || !v.keepDeltas)
        return fail(c, DOPF_E_UNSUPPORTED, "the agents' injection changes are kept on the device only with lines and DOPF_F_KEEP_DELTAS "
                                           "(otherwise: dopf_get_agent_penalty with the change passed in, agent by agent)");
    DeviceGuard guard(c->device);
    const size_t NT = (size_t)v.N * v.T;
    double *tmp = nullptr;
    int rc = getter_scratch(c, &tmp);
    if (rc) return rc;
    launch_penalty_sums(v, tmp, c->main);
    HIPCHK(c, hipGetLastError());
    std::vector<double> h(3 * NT);
    HIPCHK(c, hipMemcpyAsync(h.data(), tmp, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    for (int k = 0; k < 3; ++k)
        for (int t = 0; t < v.T; ++t) {
            double sum = 0.0;
            for (int n = 0; n < v.N; ++n) sum += h[k * NT + (size_t)n * v.T + t];       // (node order: fixed)
            penalty[(size_t)k * v.T + t] = sum;
        }
    return DOPF_OK;
}

int dopf_set_state(dopf_ctx *c, const double *P, const double *D, const double *C, const double *avg_U,
                   const double *avg_K, const double *lambda, const double *mu, const double *rho, int32_t iteration)
{
    if (!c || iteration < 1) return fail(c, DOPF_E_INVALID, "bad argument");
    DeviceGuard guard(c->device);
    DevView &v = c->v;
    const size_t LT = (size_t)v.L * v.T;
    HIPCHK(c, hipStreamSynchronize(c->main));
    int rc;
    if ((rc = set_rows(c, v.P, P, c->gen_perm))) return rc;
    if ((rc = set_rows(c, v.D, D, c->sto_perm))) return rc;
    if ((rc = set_rows(c, v.C, C, c->sto_perm))) return rc;
    auto up = [&](double *dst, const double *src, size_t n) -> int {
        if (!src || n == 0) return DOPF_OK;
        HIPCHK(c, hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice));
        return DOPF_OK;
    };
    if ((rc = up(v.avgU, avg_U, LT))) return rc;
    if ((rc = up(v.avgK, avg_K, LT))) return rc;
    if ((rc = up(v.lam, lambda, v.T))) return rc;
    if ((rc = up(v.mu, mu, LT))) return rc;
    if ((rc = up(v.rho, rho, LT))) return rc;
    if (v.S > 0) HIPCHK(c, hipMemset(v.nu_valid, 0, sizeof(int) * v.S));   // stored prices no longer match the state
    if (v.G > 0 && P) {                                                     // nor do the row summaries of P
        std::vector<int> mixed(v.G, 2);
        HIPCHK(c, hipMemcpy(v.gen_state, mixed.data(), sizeof(int) * v.G, hipMemcpyHostToDevice));
    }
    c->quiet = false;                      // (flags are formed anew from the state handed in)
    Status st{};
    HIPCHK(c, hipMemcpy(&st, v.st, sizeof st, hipMemcpyDeviceToHost));
    st.iteration = iteration;
    st.converged = 0;
    st.halt = (v.max_iters > 0 && iteration > v.max_iters);
    st.resbits[0] = st.resbits[1] = st.resbits[2] = 0;
    memset(st.resbits2, 0, sizeof st.resbits2);
    HIPCHK(c, hipMemcpy(v.st, &st, sizeof st, hipMemcpyHostToDevice));
    launch_derive(v, c->plan, c->main, true);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->main));
    c->host_st = st;
    return DOPF_OK;
}

// Convergence.{lambda_res, mue_res, rho_res}[end] (src/structures/convergence.jl:5-12, src/optimization/convergence.jl:5-13):
// |dual after the last update - dual the last solve used|, entry by entry
int dopf_get_residual_vectors(dopf_ctx *c, double *lam_res, double *mu_res, double *rho_res)
{
    if (!c) return DOPF_E_INVALID;
    const size_t T = c->v.T, LT = (size_t)c->v.L * c->v.T;
    std::vector<double> a(std::max(T, LT)), b(std::max(T, LT));
    auto diff = [&](double *out, const double *now, const double *used, size_t n) -> int {
        if (!out || n == 0) return DOPF_OK;
        DeviceGuard guard(c->device);
        HIPCHK(c, hipMemcpyAsync(a.data(), now, n * sizeof(double), hipMemcpyDeviceToHost, c->main));
        HIPCHK(c, hipMemcpyAsync(b.data(), used, n * sizeof(double), hipMemcpyDeviceToHost, c->main));
        HIPCHK(c, hipStreamSynchronize(c->main));
        for (size_t i = 0; i < n; ++i) out[i] = fabs(a[i] - b[i]);
        return DOPF_OK;
    };
    int rc;
    if ((rc = diff(lam_res, c->v.lam, c->v.lam_used, T))) return rc;
    if ((rc = diff(mu_res, c->v.mu, c->v.mu_used, LT))) return rc;
    return diff(rho_res, c->v.rho, c->v.rho_used, LT);
}

// ResultGenerator/ResultStorage.{U, K, penalty_term} of the last solve (src/structures/results.jl:1-17,
// src/optimization/penalty_terms.jl:1-37): not stored per agent on the device — the slacks are eliminated in closed
// form — but recomputed here from the agent's injection change and the consensus state that solve read.
static int agent_result(dopf_ctx *c, int32_t agent, const double *delta_in, double *U, double *K, double *pen)
{
    const DevView &v = c->v;
    const int T = v.T, L = v.L, N = v.N, G = v.G, S = v.S;
    if (agent < 0 || agent >= G + S) return fail(c, DOPF_E_INVALID, "agent %d of %d", agent, G + S);
    if (!delta_in && L == 0) {
        if (pen) return fail(c, DOPF_E_UNSUPPORTED, "copper plate: the agent's injection change is not kept on the device (pass it in)");
        return DOPF_OK;         // no lines: U and K are empty
    }
    if (!delta_in && !v.keepDeltas)
        return fail(c, DOPF_E_UNSUPPORTED, "the agents' injection changes are kept on the device only with DOPF_F_KEEP_DELTAS (or pass the change in)");
    DeviceGuard guard(c->device);
    const bool is_gen = agent < G;
    const std::vector<int> &perm = is_gen ? c->gen_perm : c->sto_perm;
    const int want = is_gen ? agent : agent - G;
    int row = -1;
    for (size_t i = 0; i < perm.size(); ++i) if (perm[i] == want) { row = (int)i; break; }
    if (row < 0) return fail(c, DOPF_E_INVALID, "agent not found");
    HIPCHK(c, hipStreamSynchronize(c->main));
    // node of the agent: the item lists are per node; read it from the node ranges
    std::vector<int> beg(N + 1);
    HIPCHK(c, hipMemcpy(beg.data(), is_gen ? v.node_gen_beg : v.node_sto_beg, sizeof(int) * (N + 1), hipMemcpyDeviceToHost));
    int n = 0;
    while (n + 1 < N && row >= beg[n + 1]) ++n;
    std::vector<double> dl(T), s(T), f((size_t)L * T), aU((size_t)L * T), aK((size_t)L * T), h(L), F(v.fmax_ld ? (size_t)L * T : (size_t)L);
    if (delta_in) memcpy(dl.data(), delta_in, sizeof(double) * T);
    else HIPCHK(c, hipMemcpy(dl.data(), (is_gen ? v.dltG : v.dltS) + (size_t)row * T, sizeof(double) * T, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(s.data(), v.s_used, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (L > 0) {
        const size_t LT = (size_t)L * T;
        HIPCHK(c, hipMemcpy(f.data(), v.flow_used, sizeof(double) * LT, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(aU.data(), v.avgU_used, sizeof(double) * LT, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(aK.data(), v.avgK_used, sizeof(double) * LT, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(h.data(), v.ptdf + (size_t)L * n, sizeof(double) * L, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(F.data(), v.fmax, sizeof(double) * F.size(), hipMemcpyDeviceToHost));
    }
    const double w2 = 2.0 * v.w_flow, g = v.gamma;
    for (int t = 0; t < T; ++t) {
        double up = 0.0, lo = 0.0;
        for (int l = 0; l < L; ++l) {
            const size_t i = l + (size_t)L * t;
            const double Fl = F[l + (size_t)v.fmax_ld * t];
            const double fl = f[i] + h[l] * dl[t];
            const double u = std::max(0.0, (g * aU[i] - w2 * (fl - Fl)) / (w2 + g));
            const double k = std::max(0.0, (g * aK[i] + w2 * (fl + Fl)) / (w2 + g));
            if (U) U[i] = u;
            if (K) K[i] = k;
            up += (fl + u - Fl) * (fl + u - Fl);                                               // penalty_terms.jl:10-20
            lo += (k - fl - Fl) * (k - fl - Fl);                                               // :23-37
        }
        if (pen) { pen[t] = (s[t] + dl[t]) * (s[t] + dl[t]); pen[T + t] = up; pen[2 * T + t] = lo; }   // :3-7
    }
    return DOPF_OK;
}

int dopf_get_agent_slacks(dopf_ctx *c, int32_t agent, double *U, double *K)
{
    if (!c) return DOPF_E_INVALID;
    return agent_result(c, agent, nullptr, U, K, nullptr);
}

int dopf_get_agent_penalty(dopf_ctx *c, int32_t agent, const double *delta, double *penalty)
{
    if (!c || !penalty) return DOPF_E_INVALID;
    return agent_result(c, agent, delta, nullptr, nullptr, penalty);
}

// diagnostics: the breakpoint table of Psi_{n,t} as the last x-update saw it (L > 0 only)
int dopf_debug_table(dopf_ctx *c, int32_t n, int32_t t, double *beta, double *psi, double *slope, double *psi0, int32_t *m)
{
    if (!c || c->v.L == 0 || n < 0 || n >= c->v.N || t < 0 || t >= c->v.T) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    const DevView &v = c->v;
    const size_t at = (size_t)n + (size_t)v.N * t;
    HIPCHK(c, hipStreamSynchronize(c->main));
    HIPCHK(c, hipMemcpy(beta, v.tb_beta + at * v.M2, sizeof(double) * v.M2, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(psi, v.tb_psi + at * v.M2, sizeof(double) * v.M2, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(slope, v.tb_slope + at * (v.M2 + 1), sizeof(double) * (v.M2 + 1), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(psi0, v.tb_psi0 + at, sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(m, v.tb_m + at, sizeof(int), hipMemcpyDeviceToHost));
    return DOPF_OK;
}

// diagnostics (DOPF_STATS builds): cumulative storage-kernel counters {scans, wave loop trips, events}
int dopf_wide_net(const dopf_ctx *c, int32_t *out)
{
    if (!c || !out) return DOPF_E_INVALID;
    *out = c->plan.wideNet ? 1 : 0;
    return DOPF_OK;
}

// The per-agent setters' common step. h holds the defaults in the context's sorted order, perm.size() values per array; a caller's
// array (a, then b behind it; NULL: the default stays) overwrites them through the permutation (+ 0.0: a -0.0 is stored as 0.0). One
// copy to dst, ordered on the context's stream behind what is queued there; the graphs read the same device array (no capture again).
// h must outlive the copy: the setter synchronises before it returns.
static int stage_and_copy(dopf_ctx *c, const std::vector<int> &perm, std::vector<double> &h, const double *a, const double *b, const double *dst)
{
    const size_t n = perm.size();
    for (size_t i = 0; i < n; ++i) {
        if (a) h[i] = a[perm[i]] + 0.0;
        if (b) h[n + i] = b[perm[i]] + 0.0;
    }
    HIPCHK(c, hipMemcpyAsync(const_cast<double *>(dst), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->main));
    return DOPF_OK;
}

// The storage setters' common step: `n` slots of the storage block from slot `first` on (dopf_internal.h: StoSlot) take the caller's arrays
// a and b (NULL: the slot's default), on the device and in the context's mirror
static int set_sto_slots(dopf_ctx *c, int first, int n, const double *a, const double *b)
{
    const size_t S = (size_t)c->v.S;
    DeviceGuard guard(c->device);
    std::vector<double> h((size_t)n * S);
    for (int k = 0; k < n; ++k)
        for (size_t i = 0; i < S; ++i) h[k * S + i] = sto_slot_default(first + k, c->sto_at(kStoEmax, (int)i));
    if (int rc = stage_and_copy(c, c->sto_perm, h, a, b, sto_slot(c->v, first))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main));
    std::copy(h.begin(), h.end(), c->sto_slot_h(first));          // (what the other setters check reachability against)
    return DOPF_OK;
}

int dopf_set_storage_initial_level(dopf_ctx *c, const double *e0)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_initial_levels(c, e0)) return rc;
    if (c->v.S == 0) return DOPF_OK;
    return set_sto_slots(c, kStoE0, 1, e0, nullptr);
}

int dopf_set_storage_terminal_level(dopf_ctx *c, const double *lo, const double *hi)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_terminal_levels(c, lo, hi)) return rc;
    if (c->v.S == 0) return DOPF_OK;
    return set_sto_slots(c, kStoEndLo, 2, lo, hi);
}

int dopf_set_storage_efficiency(dopf_ctx *c, const double *eta_c, const double *eta_d)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_storage_efficiency(c, eta_c, eta_d)) return rc;
    const int S = c->v.S;
    if (S == 0) return DOPF_OK;
    std::vector<double> al;
    if (eta_d) {
        al.resize(S);
        for (int a = 0; a < S; ++a) al[a] = 1.0 / eta_d[a];
    }
    return set_sto_slots(c, kStoAlpha, 2, eta_d ? al.data() : nullptr, eta_c);
}

// a checked table and the generators' indices (pr: sorted order) on their way to the device, on the context's stream; the caller
// synchronises before profiles and pr go, and keeps the host mirrors (dopf_set_generator_availability, dopf_roll_horizon_coupled)
static int queue_availability(dopf_ctx *c, int32_t n_profiles, const double *profiles, const std::vector<int> &pr)
{
    DevView &v = c->v;
    const int G = v.G, T = v.T;
    const size_t need = (size_t)n_profiles * T;
    if (n_profiles > c->gen_avail_cap) {
        // the table grows: a new allocation, whose address goes into gen_avail_slot(v) behind everything queued (the kernels read it
        // there, once per block). The iteration graphs are captured again at the next dopf_iterate. (The old table stays allocated
        // until the context goes.)
        HIPCHK(c, hipStreamSynchronize(c->main));
        const int cap = std::max(n_profiles, 2 * c->gen_avail_cap);
        double *tab = nullptr;
        if (int rc = dev_alloc(c, &tab, (size_t)cap * T, false)) return rc;
        c->gen_avail = tab;
        c->gen_avail_cap = cap;
        HIPCHK(c, hipMemcpyAsync(gen_avail_slot(v), &c->gen_avail, sizeof(double *), hipMemcpyHostToDevice, c->main));
        drop_graphs(c);
    }
    // ordered on the context's stream behind what is queued there: the table, the indices, and the rows that sat at their old caps
    // (state 1) demoted to "mixed" — at the new caps they are not (state 0 stays: a row at 0 is at 0 under any cap >= 0)
    if (need) HIPCHK(c, hipMemcpyAsync(c->gen_avail, profiles, need * sizeof(double), hipMemcpyHostToDevice, c->main));
    HIPCHK(c, hipMemcpyAsync(gen_prof(v), pr.data(), sizeof(int) * G, hipMemcpyHostToDevice, c->main));
    launch_demote_full_rows(v, c->main);
    HIPCHK(c, hipGetLastError());
    return DOPF_OK;
}

int dopf_set_generator_availability(dopf_ctx *c, int32_t n_profiles, const double *profiles, const int32_t *profile_of)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_availability(c, n_profiles, profiles, profile_of)) return rc;
    const int G = c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    std::vector<int> pr(G, -1);
    if (profile_of)
        for (int i = 0; i < G; ++i) pr[i] = profile_of[c->gen_perm[i]];
    const size_t need = (size_t)n_profiles * c->v.T;
    if (int rc = queue_availability(c, n_profiles, profiles, pr)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->main));
    c->gen_prof_h = pr;
    if ((c->q.flags & DOPF_F_GEN_RAMP) || (c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET)) c->gen_avail_h.assign(profiles, profiles + need);      // (what dopf_set_generator_ramp checks its anchors against, dopf_set_generator_energy_budget its minima)
    return DOPF_OK;
}

int dopf_set_line_rating(dopf_ctx *c, const double *rating)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_line_rating(c, rating)) return rc;
    DevView &v = c->v;
    const int L = v.L, T = v.T;
    if (L == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    const size_t LT = (size_t)L * T;
    // ordered on the context's stream behind what is queued there; the graphs read the same device array (no capture again). NULL:
    // the limits of dopf_create (kept behind the table) in every timestep. Then the derived state of the consensus step — the
    // per-(l,t) flags of the slack sums among it — is formed again under the new limits, from the sums the last iteration left in
    // the consensus buffer (on a communicator: the summed ones, the same on every rank; nothing is summed or exchanged here)
    if (rating) {
        HIPCHK(c, hipMemcpyAsync(const_cast<double *>(v.fmax), rating, LT * sizeof(double), hipMemcpyHostToDevice, c->main));
        HIPCHK(c, hipStreamSynchronize(c->main));           // (the caller's array is the caller's again at return)
    } else {
        for (int t = 0; t < T; ++t)
            HIPCHK(c, hipMemcpyAsync(const_cast<double *>(v.fmax) + (size_t)L * t, line_fmax0(v), L * sizeof(double), hipMemcpyDeviceToDevice, c->main));
    }
    launch_line_rating(v, c->plan, c->main);
    HIPCHK(c, hipGetLastError());
    c->quiet = false;                      // (flags are formed anew under the new limits)
    return read_status(c);
}

int dopf_set_generator_quadratic_cost(dopf_ctx *c, const double *c2)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_quadratic_cost(c, c2)) return rc;
    const int G = c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    std::vector<double> h(G, 0.0);
    // the state stays; the stop test starts over, as after dopf_set_line_rating (nothing derived depends on the costs)
    if (int rc = stage_and_copy(c, c->gen_perm, h, c2, nullptr, gen_c2(c->v))) return rc;
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    return read_status(c);          // (synchronises: h may go)
}

int dopf_set_generator_ramp(dopf_ctx *c, const double *up, const double *down, const double *prev)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_ramp(c, up, down, prev)) return rc;
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    std::vector<double> h(3 * G, INFINITY);
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        if (up) { h[i] = up[a] + 0.0; h[G + i] = down[a] + 0.0; }
        h[2 * G + i] = prev ? prev[a] + 0.0 : std::nan("");
    }
    // ordered on the context's stream behind what is queued there; the graphs read the same device array (no capture again). The
    // state stays; the stop test starts over, as after dopf_set_generator_quadratic_cost
    HIPCHK(c, hipMemcpyAsync(const_cast<double *>(gen_ramp_up(c->v)), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->main));
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    if (int rc = read_status(c)) return rc;          // (synchronises: h may go)
    std::copy(h.begin(), h.end(), c->gen_ramp_h.begin() + G);
    return DOPF_OK;
}

int dopf_set_generator_min_output(dopf_ctx *c, const double *p_min)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_min_output(c, p_min)) return rc;
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    std::vector<double> h(G, 0.0);
    if (p_min)
        for (size_t i = 0; i < G; ++i) h[i] = p_min[c->gen_perm[i]] + 0.0;
    // the first array switches the context to the MN instantiations of its generator kernel, NULL switches back: other kernels, so the
    // iteration graphs are captured again at the next dopf_iterate (as after a grown availability table). Between two arrays the graphs
    // read the same device array (no capture again)
    const bool on = p_min != nullptr;
    if (on != c->plan.genMinOut) {
        HIPCHK(c, hipStreamSynchronize(c->main));
        c->plan.genMinOut = on;
        drop_graphs(c);
    }
    // ordered on the context's stream behind what is queued there. The state stays (a P below its floor is a proximal centre: the next
    // x-update clamps it); the stop test starts over, as after dopf_set_generator_ramp
    HIPCHK(c, hipMemcpyAsync(const_cast<double *>(gen_min_output(c->v)), h.data(), G * sizeof(double), hipMemcpyHostToDevice, c->main));
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    if (int rc = read_status(c)) return rc;          // (synchronises: h may go)
    c->gen_min_h = h;
    return DOPF_OK;
}

// the stored floors from the host mirror (no device call); a context without DOPF_F_GEN_RAMP holds none: zeros
int dopf_get_generator_min_output(dopf_ctx *c, double *p_min)
{
    if (!c) return DOPF_E_INVALID;
    if (!p_min) return c->v.G == 0 ? DOPF_OK : fail(c, DOPF_E_INVALID, "dopf_get_generator_min_output: p_min is NULL");
    for (int i = 0; i < c->v.G; ++i) p_min[c->gen_perm[i]] = c->gen_min_h.empty() ? 0.0 : c->gen_min_h[(size_t)i];
    return DOPF_OK;
}

// the floors of a budget context. The device array is the context's own, allocated and zeroed at the first call with an
// array and kept from then on (Plan::genBudgetMinOut points at it while floors are set)
int dopf_set_generator_budget_min_output(dopf_ctx *c, const double *p_min)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_budget_min_output(c, p_min)) return rc;
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    if (!p_min && !c->gen_bmin_d) {                        // (no floors were ever set: nothing to take back but the stop test)
        launch_reset_status(c->v, c->main);
        HIPCHK(c, hipGetLastError());
        return read_status(c);
    }
    std::vector<double> h(G, 0.0);
    if (p_min)
        for (size_t i = 0; i < G; ++i) h[i] = p_min[c->gen_perm[i]] + 0.0;
    if (!c->gen_bmin_d) {
        const unsigned long long need = (unsigned long long)G * sizeof(double);
        HIPCHK(c, hipStreamSynchronize(c->main));
        size_t freeb = 0, totalb = 0;
        HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
        if (need > freeb)
            return fail(c, DOPF_E_NOMEM, "dopf_set_generator_budget_min_output: the floors (G doubles) need %llu bytes, the device has %llu free", need,
                        (unsigned long long)freeb);
        if (int rc = dev_alloc(c, &c->gen_bmin_d, G, true)) return rc;      // (zeroed on the context's stream, as the ramp prices are)
    }
    // the first array switches the context to the MN instantiations of its generator kernel, NULL switches back: other kernels, so the
    // iteration graphs are captured again at the next dopf_iterate. Between two arrays the graphs read the same device array
    const bool on = p_min != nullptr;
    if (on != (c->plan.genBudgetMinOut != nullptr)) {
        HIPCHK(c, hipStreamSynchronize(c->main));
        c->plan.genBudgetMinOut = on ? c->gen_bmin_d : nullptr;
        drop_graphs(c);
    }
    // ordered on the context's stream behind what is queued there. The state stays (a P below its floor is a proximal centre: the next
    // x-update clamps it); the stop test starts over, as after dopf_set_generator_min_output
    HIPCHK(c, hipMemcpyAsync(c->gen_bmin_d, h.data(), G * sizeof(double), hipMemcpyHostToDevice, c->main));
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    if (int rc = read_status(c)) return rc;          // (synchronises: h may go)
    c->gen_bmin_h = h;
    return DOPF_OK;
}

// the stored floors from the host mirror (no device call); a context that never set any holds none: zeros
int dopf_get_generator_budget_min_output(dopf_ctx *c, double *p_min)
{
    if (!c) return DOPF_E_INVALID;
    if (!p_min) return c->v.G == 0 ? DOPF_OK : fail(c, DOPF_E_INVALID, "dopf_get_generator_budget_min_output: p_min is NULL");
    for (int i = 0; i < c->v.G; ++i) p_min[c->gen_perm[i]] = c->gen_bmin_h.empty() ? 0.0 : c->gen_bmin_h[(size_t)i];
    return DOPF_OK;
}

// the multipliers of the last computed x-update, as k_gen_budget<.., PR = true> / k_gen_ramp_budget stored them (sorted order on the device)
int dopf_get_generator_budget_price(dopf_ctx *c, double *nu)
{
    if (!c) return DOPF_E_INVALID;
    if (!(c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET))
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_get_generator_budget_price: the context was created without DOPF_F2_GEN_ENERGY_BUDGET");
    if (!c->gen_bw_end_h.empty())
        return fail(c, DOPF_E_INVALID, "dopf_get_generator_budget_price: the context holds budgets per sub-window (n_win = %d), whose prices "
                                       "dopf_get_generator_budget_window_price returns", (int)c->gen_bw_end_h.size());
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    if (!nu) return fail(c, DOPF_E_INVALID, "dopf_get_generator_budget_price: nu is NULL");
    DeviceGuard guard(c->device);
    // the first call switches a budget context to the PR instantiations of k_gen_budget, which store the prices (the store costs
    // time: DESIGN.md 5za): other kernels, so the iteration graphs are captured again at the next dopf_iterate, as after the first
    // dopf_set_generator_min_output. The pair's kernel (DOPF_F2_GEN_RAMP_BUDGET) always stores: nothing to switch there
    if (c->plan.genBudget && !c->plan.genRampBudget && !c->plan.genBudgetPrice) {
        HIPCHK(c, hipStreamSynchronize(c->main));
        c->plan.genBudgetPrice = true;
        drop_graphs(c);
    }
    std::vector<double> h(G);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->gen_budget_price_d(), G * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    for (size_t i = 0; i < G; ++i) nu[c->gen_perm[i]] = h[i];
    return DOPF_OK;
}

// the ramp rows' multipliers of the last computed x-update, as k_gen_ramp<.., RP = true> / k_gen_ramp_budget<.., RP = true> stored
// them (sorted order on the device, T per row); the array is the context's own, allocated by the first call
int dopf_get_generator_ramp_price(dopf_ctx *c, double *rp)
{
    if (!c) return DOPF_E_INVALID;
    if (!(c->q.flags & DOPF_F_GEN_RAMP))
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_get_generator_ramp_price: the context was created without DOPF_F_GEN_RAMP");
    if (c->v.L > 0)
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_get_generator_ramp_price: network rows are not priced (k_gen_ramp_net keeps no centre, and a "
                                           "row's gradient there needs the node's table); L = %d", c->v.L);
    const size_t G = (size_t)c->v.G, T = (size_t)c->v.T;
    if (G == 0) return DOPF_OK;
    if (!rp) return fail(c, DOPF_E_INVALID, "dopf_get_generator_ramp_price: rp is NULL");
    DeviceGuard guard(c->device);
    // the first call: the array, zeroed, and the RP instantiations of the context's generator kernel — other kernels, so the iteration
    // graphs are captured again at the next dopf_iterate, as after the first dopf_set_generator_min_output. No way back
    if (!c->plan.genRampPrice) {
        const unsigned long long need = (unsigned long long)G * T * sizeof(double);
        HIPCHK(c, hipStreamSynchronize(c->main));
        size_t freeb = 0, totalb = 0;
        HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
        if (need > freeb)
            return fail(c, DOPF_E_NOMEM, "dopf_get_generator_ramp_price: the ramp prices (T x G doubles) need %llu bytes, the device has %llu free",
                        need, (unsigned long long)freeb);
        // dev_alloc, as every other array of the context: under DOPF_GUARD the block ends on the last bytes of its own mapping, and it
        // is zeroed on the context's stream — c->main does not wait for the null stream (hipStreamNonBlocking), so a hipMemset there
        // would not be ordered before the copy below, which then returns what the block held before
        double *p = nullptr;
        if (int rc = dev_alloc(c, &p, G * T, true)) return rc;
        c->plan.genRampPrice = p;
        drop_graphs(c);
    }
    std::vector<double> h(G * T);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->plan.genRampPrice, G * T * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    for (size_t i = 0; i < G; ++i) std::copy(h.begin() + i * T, h.begin() + (i + 1) * T, rp + (size_t)c->gen_perm[i] * T);
    return DOPF_OK;
}

int dopf_set_generator_energy_budget(dopf_ctx *c, const double *e_min, const double *e_max)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_energy_budget(c, e_min, e_max)) return rc;
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    std::vector<double> h(2 * G);
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        h[i] = e_min ? e_min[a] + 0.0 : 0.0;
        h[G + i] = e_max ? e_max[a] + 0.0 : INFINITY;
    }
    // ordered on the context's stream behind what is queued there; the graphs read the same device array (no capture again). The
    // state stays; the stop test starts over, as after dopf_set_generator_ramp
    // (DOPF_F2_GEN_RAMP_BUDGET: the budgets sit behind the ramps and the anchor)
    const double *dst = c->plan.genRampBudget ? gen_rb_min(c->v) : gen_budget_min(c->v);
    HIPCHK(c, hipMemcpyAsync(const_cast<double *>(dst), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->main));
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    if (int rc = read_status(c)) return rc;          // (synchronises: h may go)
    std::copy(h.begin(), h.end(), c->gen_budget_h.begin() + G);
    return DOPF_OK;
}

// the device block of a table of n_win windows: prices | e_min | e_max (n_win x G doubles each, sorted order) | the ends (n_win ints)
static void budget_win_view(dopf::BudgetWinView *bw, void *blk, size_t G, int n_win)
{
    const size_t n = G * (size_t)n_win;
    double *d = (double *)blk;
    bw->nu = d;
    bw->emin = d + n;
    bw->emax = d + 2 * n;
    bw->end = (const int *)(d + 3 * n);
    bw->n_win = n_win;
}

static void budget_win_release(dopf_ctx *c)
{
    if (!c->gen_bw_base) return;
    auto it = std::find(c->allocs.begin(), c->allocs.end(), c->gen_bw_base);
    if (it != c->allocs.end()) c->allocs.erase(it);
    hipFree(c->gen_bw_base);
    c->gen_bw_base = nullptr;
}

int dopf_set_generator_energy_budget_windows(dopf_ctx *c, int32_t n_win, const int32_t *win_end, const double *e_min, const double *e_max)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = check_generator_energy_budget_windows(c, n_win, win_end, e_min, e_max)) return rc;
    const size_t G = (size_t)c->v.G;
    if (G == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    const int stored = (int)c->gen_bw_end_h.size();
    const size_t n = G * (size_t)n_win;
    std::vector<double> h(2 * n);
    for (size_t i = 0; i < G; ++i) {
        const size_t a = (size_t)c->gen_perm[i];
        for (size_t j = 0; j < (size_t)n_win; ++j) {
            h[j + n_win * i] = e_min ? e_min[j + n_win * a] + 0.0 : 0.0;
            h[n + j + n_win * i] = e_max ? e_max[j + n_win * a] + 0.0 : INFINITY;
        }
    }
    if (n_win != stored) {
        // another kernel (the first table, none) or other arrays behind its second argument: the stream drains, the block is replaced
        // and the iteration graphs are captured again at the next dopf_iterate
        HIPCHK(c, hipStreamSynchronize(c->main));
        void *blk = nullptr;
        if (n_win > 0) {
            const unsigned long long need = 3ull * n * sizeof(double) + (unsigned long long)n_win * sizeof(int);
            size_t freeb = 0, totalb = 0;
            HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
            if (need > freeb)
                return fail(c, DOPF_E_NOMEM, "dopf_set_generator_energy_budget_windows: the table (n_win = %d ends, 3 x n_win x G doubles) needs %llu bytes, "
                                             "the device has %llu free", n_win, need, (unsigned long long)freeb);
            char *q = nullptr;
            if (int rc = dev_alloc(c, &q, (size_t)need, false)) return rc;
            blk = c->allocs.back();
            budget_win_release(c);
            c->gen_bw_base = blk;
            budget_win_view(&c->plan.genBudgetWin, q, G, n_win);
            HIPCHK(c, hipMemsetAsync(c->plan.genBudgetWin.nu, 0, n * sizeof(double), c->main));
        } else {
            budget_win_release(c);
            c->plan.genBudgetWin = dopf::BudgetWinView{};
        }
        drop_graphs(c);
    }
    // ordered on the context's stream behind what is queued there; with the same n_win the graphs read the same device arrays (no
    // capture again). The state stays; the stop test starts over, as after dopf_set_generator_energy_budget
    if (n_win > 0) {
        const dopf::BudgetWinView &bw = c->plan.genBudgetWin;
        HIPCHK(c, hipMemcpyAsync(const_cast<double *>(bw.emin), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->main));
        HIPCHK(c, hipMemcpyAsync(const_cast<int *>(bw.end), win_end, (size_t)n_win * sizeof(int), hipMemcpyHostToDevice, c->main));
    }
    launch_reset_status(c->v, c->main);
    HIPCHK(c, hipGetLastError());
    if (int rc = read_status(c)) return rc;          // (synchronises: h and win_end may go)
    c->gen_bw_end_h.assign(win_end, win_end + n_win);
    c->gen_bw_h = h;
    return DOPF_OK;
}

// the stored table from the host mirrors (no device call)
int dopf_get_generator_energy_budget_windows(dopf_ctx *c, int32_t *n_win, int32_t *win_end, double *e_min, double *e_max)
{
    if (!c) return DOPF_E_INVALID;
    const size_t nw = c->gen_bw_end_h.size(), G = (size_t)c->v.G, n = nw * G;
    if (n_win) *n_win = (int32_t)nw;
    if (win_end) std::copy(c->gen_bw_end_h.begin(), c->gen_bw_end_h.end(), win_end);
    for (size_t i = 0; i < G && nw > 0; ++i) {
        const size_t a = (size_t)c->gen_perm[i];
        if (e_min) std::copy(c->gen_bw_h.begin() + nw * i, c->gen_bw_h.begin() + nw * (i + 1), e_min + nw * a);
        if (e_max) std::copy(c->gen_bw_h.begin() + n + nw * i, c->gen_bw_h.begin() + n + nw * (i + 1), e_max + nw * a);
    }
    return DOPF_OK;
}

// the windows' multipliers of the last computed x-update, as k_gen_budget_win stored them (sorted order on the device)
int dopf_get_generator_budget_window_price(dopf_ctx *c, double *nu)
{
    if (!c) return DOPF_E_INVALID;
    const size_t G = (size_t)c->v.G, nw = c->gen_bw_end_h.size();
    if (G == 0) return DOPF_OK;
    if (nw == 0)
        return fail(c, DOPF_E_INVALID, "dopf_get_generator_budget_window_price: no table is set (dopf_set_generator_energy_budget_windows first)");
    if (!nu) return fail(c, DOPF_E_INVALID, "dopf_get_generator_budget_window_price: nu is NULL");
    DeviceGuard guard(c->device);
    std::vector<double> h(G * nw);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->plan.genBudgetWin.nu, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    for (size_t i = 0; i < G; ++i) std::copy(h.begin() + nw * i, h.begin() + nw * (i + 1), nu + nw * (size_t)c->gen_perm[i]);
    return DOPF_OK;
}

// scratch of dopf_set_demand / dopf_roll_horizon, allocated at the first call (freed with the context's other arrays): the moved
// per-timestep vectors (demand, 2 x lambda, 8 line vectors, with DOPF_F_LINE_RATING the rating table) | the caller's demand tail (up to N*(T-1)) | the new initial levels (S)
// | dopf_roll_horizon_coupled: the new anchor, what is left of e_min and e_max, what was spent (G each). The offsets are formed here alone
struct RollScratch { double *vecs, *tail, *e0, *gen; };
static int roll_scratch(dopf_ctx *c, RollScratch *out)
{
    const size_t NT = (size_t)c->v.N * c->v.T, LT = (size_t)c->v.L * c->v.T, S = (size_t)c->v.S, G = (size_t)c->v.G;
    const size_t vecs = NT + 2 * (size_t)c->v.T + (c->v.fmax_ld ? 9 : 8) * LT;
    if (!c->roll_scratch) {
        int rc = dev_alloc(c, &c->roll_scratch, vecs + NT + S + 4 * G, false);
        if (rc) return rc;
    }
    out->vecs = c->roll_scratch;
    out->tail = out->vecs + vecs;
    out->e0 = out->tail + NT;
    out->gen = out->e0 + S;
    return DOPF_OK;
}

// the checks both entries share: a context of its own (no communicator), and n finite values behind p
static int roll_checks(dopf_ctx *c, const char *entry, const char *what, const double *p, size_t n, int N, int t0)
{
    if (c->comm)
        return fail(c, DOPF_E_UNSUPPORTED, "%s: not on a context joined to a communicator or a peer exchange (the shards' node sums "
                                           "would need an exchange)", entry);
    if (!p) return fail(c, DOPF_E_INVALID, "%s: %s is NULL", entry, what);
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i]))
            return fail(c, DOPF_E_INVALID, "%s: %s[%zu] (node %zu, t = %zu) is %g", entry, what, i, i % (size_t)N, i / (size_t)N + (size_t)t0, p[i]);
    return DOPF_OK;
}

int dopf_set_demand(dopf_ctx *c, const double *demand)
{
    if (!c) return DOPF_E_INVALID;
    DevView &v = c->v;
    const size_t NT = (size_t)v.N * v.T;
    if (int rc = roll_checks(c, "dopf_set_demand", "demand", demand, NT, v.N, 0)) return rc;
    DeviceGuard guard(c->device);
    // ordered on the context's stream behind what is queued there; the graphs read the same device array (no capture again). The
    // node sums are formed again from P, D and C (item by item, in parallel): every chain leaves its last sums in cons, but a
    // buffer bound by the caller (dopf_bind_consensus) holds whatever the caller left in it; as dopf_set_state does — DESIGN.md 5l
    HIPCHK(c, hipMemcpyAsync(const_cast<double *>(v.demand), demand, NT * sizeof(double), hipMemcpyHostToDevice, c->main));
    launch_roll_state(v, c->plan, 0, 0, c->main);
    HIPCHK(c, hipGetLastError());
    c->quiet = false;                      // (flags are formed anew from the new flows)
    return read_status(c);
}

// what dopf_roll_horizon_coupled takes beyond dopf_roll_horizon's arguments
struct RollCoupling {
    int32_t n_profiles;                    // -1: the stored table stays
    const double *profiles;
    const int32_t *profile_of;
    int32_t set_budget;                    // != 0: e_min / e_max are the new window's budgets (NULL: 0 / +inf)
    const double *e_min, *e_max;
};

// the generators' host mirrors as the next window will have them, in the shapes the context keeps (sorted order). The setters' checks
// read the context's mirrors, so the roll's checks run with these swapped in, and they are swapped in for good once the commit is queued
struct GenWindow {
    std::vector<double> ramp, budget, avail;
    std::vector<int> prof;
    void swap(dopf_ctx *c) { c->gen_ramp_h.swap(ramp); c->gen_budget_h.swap(budget); c->gen_avail_h.swap(avail); c->gen_prof_h.swap(prof); }
};

// the three setters' checks on the next window: the new anchor under the stored ramps, the new budgets, both under the table that
// will be in force, and with DOPF_F2_GEN_RAMP_BUDGET every row's joint feasibility. The context's mirrors are as before at return
static int check_gen_window(dopf_ctx *c, const char *entry, GenWindow &w)
{
    const size_t G = (size_t)c->v.G;
    const bool ramp = c->plan.genRamp, budget = c->plan.genBudget;
    std::vector<double> up, down, prev, lo, hi;          // (the checks read the caller's order)
    if (ramp) { up.resize(G); down.resize(G); prev.resize(G); }
    if (budget) { lo.resize(G); hi.resize(G); }
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        if (ramp) { up[a] = w.ramp[G + i]; down[a] = w.ramp[2 * G + i]; prev[a] = w.ramp[3 * G + i]; }
        if (budget) { lo[a] = w.budget[G + i]; hi[a] = w.budget[2 * G + i]; }
    }
    w.swap(c);
    int rc = DOPF_OK;
    if (ramp) rc = check_generator_ramp_values(c, entry, c->gen_ramp_h.data(), c->gen_avail_h.data(), up.data(), down.data(), prev.data());
    if (!rc && budget) rc = check_generator_energy_budget_values(c, entry, c->gen_budget_h.data(), c->gen_avail_h.data(), lo.data(), hi.data());
    if (!rc) rc = ramp_floor_rows_fit(c, entry, nullptr, false, nullptr, nullptr, nullptr, false, nullptr, nullptr);     // (the stored floors stay)
    if (!rc) rc = budget_floor_rows_fit(c, entry, BudgetFloorGiven{});     // (the stored floors of dopf_set_generator_budget_min_output stay too)
    if (!rc) rc = ramp_budget_rows_fit(c, entry, false, nullptr, nullptr, nullptr, false, nullptr, nullptr, false, nullptr, nullptr);
    w.swap(c);
    return rc;
}

// the body of dopf_roll_horizon and dopf_roll_horizon_coupled (cp: the latter's inputs, null for the former, whose caller has refused
// the contexts with an anchor or a budget)
static int roll_window(dopf_ctx *c, const char *entry, int32_t k, const double *demand_tail, const RollCoupling *cp)
{
    DevView &v = c->v;
    const int N = v.N, L = v.L, T = v.T, S = v.S;
    const size_t G = (size_t)v.G;
    if (k < 1 || k >= T) return fail(c, DOPF_E_INVALID, "%s: k = %d outside [1, T - 1 = %d]", entry, k, T - 1);
    if (int rc = roll_checks(c, entry, "demand_tail", demand_tail, (size_t)N * k, N, T - k)) return rc;
    if (S > 0 && !(c->q.flags & DOPF_F_STO_INITIAL_LEVEL))
        return fail(c, DOPF_E_UNSUPPORTED, "%s: the storages' levels after %d steps become the next window's initial levels, "
                                           "which need DOPF_F_STO_INITIAL_LEVEL at dopf_create", entry, k);
    // the generator part: the anchor, what is left of the stored budgets (or the caller's new ones), the caller's table
    const bool ramp = cp && c->plan.genRamp, budget = cp && c->plan.genBudget, table = cp && G > 0 && cp->n_profiles >= 0;
    const bool left = budget && !cp->set_budget, gens = ramp || budget || table;
    DeviceGuard guard(c->device);
    RollScratch scr{};
    if (int rc = roll_scratch(c, &scr)) return rc;
    double *const budget_d = const_cast<double *>(c->plan.genRampBudget ? gen_rb_min(v) : gen_budget_min(v));     // e_min | e_max (contexts with budgets)
    std::vector<double> e0s(S), e0c(S), gh(gens ? 3 * G : 0);
    GenWindow w;
    if (S > 0 || ramp || left) {
        // the new initial levels, anchors and budgets first, into scratch (the rows are still the old window's); checked as the setters
        // check theirs before anything is overwritten
        launch_roll_level(v, c->plan, k, !c->level_from_primal, scr.e0, c->main);
        if (ramp || left) launch_roll_gen_window(v, k, left ? budget_d : nullptr, left ? budget_d + G : nullptr, scr.gen, c->main);
        HIPCHK(c, hipGetLastError());
        if (S > 0) HIPCHK(c, hipMemcpyAsync(e0s.data(), scr.e0, sizeof(double) * S, hipMemcpyDeviceToHost, c->main));
        if (ramp) HIPCHK(c, hipMemcpyAsync(gh.data(), scr.gen, sizeof(double) * G, hipMemcpyDeviceToHost, c->main));
        if (left) HIPCHK(c, hipMemcpyAsync(gh.data() + G, scr.gen + G, sizeof(double) * 2 * G, hipMemcpyDeviceToHost, c->main));
        HIPCHK(c, hipStreamSynchronize(c->main));
    }
    if (S > 0) {
        for (int i = 0; i < S; ++i) e0c[c->sto_perm[i]] = e0s[i];          // (check_initial_levels reads the caller's order)
        if (int rc = check_initial_levels(c, e0c.data())) return rc;
    }
    if (gens) {
        w.ramp = c->gen_ramp_h; w.budget = c->gen_budget_h; w.avail = c->gen_avail_h; w.prof = c->gen_prof_h;
        for (size_t i = 0; i < G; ++i) {
            const int a = c->gen_perm[i];
            if (ramp) w.ramp[3 * G + i] = gh[i];
            if (left) { w.budget[G + i] = gh[G + i]; w.budget[2 * G + i] = gh[2 * G + i]; }
            else if (budget) { w.budget[G + i] = cp->e_min ? cp->e_min[a] + 0.0 : 0.0; w.budget[2 * G + i] = cp->e_max ? cp->e_max[a] + 0.0 : INFINITY; }
            if (table) w.prof[i] = cp->profile_of ? cp->profile_of[a] : -1;
        }
        if (table && (ramp || budget)) w.avail.assign(cp->profiles, cp->profiles + (size_t)cp->n_profiles * T);      // (kept for these contexts alone, as the setter keeps it)
        if (int rc = check_gen_window(c, entry, w)) return rc;
        // the commit, on the context's stream in the arrays the graphs read: the table as its setter queues it (a table larger than
        // any before is a new allocation, and the graphs are captured again), the anchor and the budgets from the scratch
        if (table)
            if (int rc = queue_availability(c, cp->n_profiles, cp->profiles, w.prof)) return rc;
        if (ramp) HIPCHK(c, hipMemcpyAsync(const_cast<double *>(gen_ramp_prev(v)), scr.gen, sizeof(double) * G, hipMemcpyDeviceToDevice, c->main));
        if (left) HIPCHK(c, hipMemcpyAsync(budget_d, scr.gen + G, sizeof(double) * 2 * G, hipMemcpyDeviceToDevice, c->main));
        else if (budget) HIPCHK(c, hipMemcpyAsync(budget_d, w.budget.data() + G, sizeof(double) * 2 * G, hipMemcpyHostToDevice, c->main));
    }
    HIPCHK(c, hipMemcpyAsync(scr.tail, demand_tail, sizeof(double) * N * k, hipMemcpyHostToDevice, c->main));
    RollVecs rv{};
    rv.scratch = scr.vecs;
    size_t off = 0;
    auto add = [&](double *p, int stride, const double *tail) {
        if (stride > 0) { rv.a[rv.n++] = RollVec{p, tail, off, stride}; off += (size_t)stride * T; }
    };
    add(const_cast<double *>(v.demand), N, scr.tail);
    add(v.lam, 1, nullptr); add(v.lam_used, 1, nullptr);
    for (double *p : {v.mu, v.mu_used, v.rho, v.rho_used, v.avgU, v.avgU_used, v.avgK, v.avgK_used}) add(p, L, nullptr);
    if (v.fmax_ld) add(const_cast<double *>(v.fmax), L, nullptr);          // DOPF_F_LINE_RATING: a derating persists (the old last column)
    launch_roll_vecs(rv, T, k, c->main);
    if (S > 0) {
        HIPCHK(c, hipMemcpyAsync(const_cast<double *>(sto_e0(v)), scr.e0, sizeof(double) * S, hipMemcpyDeviceToDevice, c->main));
        HIPCHK(c, hipMemsetAsync(v.nu_valid, 0, sizeof(int) * S, c->main));   // stored prices no longer match the state
    }
    if (v.G > 0) HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(v.gen_state), 2, (size_t)v.G, c->main));   // nor do the row summaries of P
    launch_roll_state(v, c->plan, k, 2, c->main);
    HIPCHK(c, hipGetLastError());
    c->quiet = false;                      // (flags are formed anew from the moved state)
    c->level_from_primal = true;           // (a central solve's levels belonged to the old window)
    if (S > 0) std::copy(e0s.begin(), e0s.end(), c->sto_slot_h(kStoE0));
    if (gens) w.swap(c);                   // (the commit is queued: a later setter's checks see the new window)
    return read_status(c);                 // (synchronises: the caller's arrays and w may go)
}

int dopf_roll_horizon(dopf_ctx *c, int32_t k, const double *demand_tail)
{
    if (!c) return DOPF_E_INVALID;
    if (c->comm) return roll_checks(c, "dopf_roll_horizon", "demand_tail", demand_tail, 0, c->v.N, 0);
    if (c->q.flags & DOPF_F_GEN_RAMP)
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_roll_horizon: not on a context with DOPF_F_GEN_RAMP (the anchor p_prev of the next window is "
                                           "the host's to set: build that window's context)");
    if (c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET)
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_roll_horizon: not on a context with DOPF_F2_GEN_ENERGY_BUDGET (what is left of a budget after "
                                           "k steps is the host's to work out: build that window's context)");
    return roll_window(c, "dopf_roll_horizon", k, demand_tail, nullptr);
}

int dopf_roll_horizon_coupled(dopf_ctx *c, int32_t k, const double *demand_tail, int32_t n_profiles, const double *profiles,
                              const int32_t *profile_of, int32_t set_budget, const double *e_min, const double *e_max)
{
    if (!c) return DOPF_E_INVALID;
    const char *entry = "dopf_roll_horizon_coupled";
    if (c->comm) return roll_checks(c, entry, "demand_tail", demand_tail, 0, c->v.N, 0);
    if (!c->gen_bw_end_h.empty())
        return fail(c, DOPF_E_UNSUPPORTED, "%s: the context holds budgets per sub-window (n_win = %d), which do not roll on the device: remove the table "
                                           "(dopf_set_generator_energy_budget_windows with n_win = 0), roll, and set the next window's table", entry,
                    (int)c->gen_bw_end_h.size());
    if (n_profiles < -1) return fail(c, DOPF_E_INVALID, "%s: n_profiles = %d < -1 (-1: the stored table stays)", entry, n_profiles);
    if (n_profiles >= 0 && !(c->q.flags & DOPF_F_GEN_AVAILABILITY))
        return fail(c, DOPF_E_UNSUPPORTED, "%s: an availability table (n_profiles = %d) needs DOPF_F_GEN_AVAILABILITY at dopf_create", entry, n_profiles);
    if (set_budget && !(c->flags2 & DOPF_F2_GEN_ENERGY_BUDGET))
        return fail(c, DOPF_E_UNSUPPORTED, "%s: set_budget = %d needs DOPF_F2_GEN_ENERGY_BUDGET at dopf_create_ex", entry, set_budget);
    if (n_profiles >= 0)
        if (int rc = check_availability_table(c, n_profiles, profiles, profile_of)) return rc;
    const RollCoupling cp{n_profiles, profiles, profile_of, set_budget, e_min, e_max};
    return roll_window(c, entry, k, demand_tail, &cp);
}

// the stored ramps, anchor and budgets from the host mirrors (no device call); without the matching flag: the defaults
int dopf_get_generator_coupling(dopf_ctx *c, double *ramp_up, double *ramp_down, double *p_prev, double *e_min, double *e_max)
{
    if (!c) return DOPF_E_INVALID;
    const size_t G = (size_t)c->v.G;
    const bool ramp = c->plan.genRamp, budget = c->plan.genBudget;
    for (size_t i = 0; i < G; ++i) {
        const int a = c->gen_perm[i];
        if (ramp_up) ramp_up[a] = ramp ? c->gen_ramp_h[G + i] : INFINITY;
        if (ramp_down) ramp_down[a] = ramp ? c->gen_ramp_h[2 * G + i] : INFINITY;
        if (p_prev) p_prev[a] = ramp ? c->gen_ramp_h[3 * G + i] : std::nan("");
        if (e_min) e_min[a] = budget ? c->gen_budget_h[G + i] : 0.0;
        if (e_max) e_max[a] = budget ? c->gen_budget_h[2 * G + i] : INFINITY;
    }
    return DOPF_OK;
}

// ---- dopf_trace_*: the iteration history on the device ---------------------------------------------------------------

static int trace_needs_active(dopf_ctx *c, const char *entry)
{
    if (c->trace.active) return DOPF_OK;
    return fail(c, DOPF_E_INVALID, "%s: no trace is active (dopf_trace_begin first)", entry);
}

int dopf_trace_begin(dopf_ctx *c, int32_t what, int32_t capacity)
{
    if (!c) return DOPF_E_INVALID;
    if (const uint32_t unknown = (uint32_t)what & ~(uint32_t)kTraceKnown)
        return fail(c, DOPF_E_INVALID, "dopf_trace_begin: what has the unknown bit %u (DOPF_TRACE_DUALS = 1, DOPF_TRACE_CONSENSUS = 2, "
                                       "DOPF_TRACE_PRIMAL = 4)", unknown & (~unknown + 1u));
    if (capacity < 1) return fail(c, DOPF_E_INVALID, "dopf_trace_begin: capacity = %d < 1", capacity);
    if (c->trace.active) return fail(c, DOPF_E_INVALID, "dopf_trace_begin: a trace is active already (dopf_trace_end first)");
    if (c->comm)
        return fail(c, DOPF_E_UNSUPPORTED, "dopf_trace_begin: not on a context joined to a communicator or a peer exchange (a sharded "
                                           "history is not recorded)");
    DeviceGuard guard(c->device);
    const DevView &v = c->v;
    dopf_ctx::Trace t{};
    t.what = what; t.capacity = capacity;
    t.lay = trace_layout(v.N, v.L, v.T, v.G, v.S, what);
    const bool levels = (what & kTracePrimal) && v.S > 0;
    t.level_slots = levels ? std::min(capacity, 64) : 0;
    // (the ring, the levels' scratch of dopf_trace_read, the trace block; a product beyond 64 bits counts as all of them)
    const unsigned __int128 need128 = (unsigned __int128)capacity * t.lay.slot_bytes +
                                      (unsigned __int128)t.level_slots * v.S * v.T * sizeof(double) + sizeof(TraceBlock);
    const unsigned long long need = need128 > (unsigned __int128)~0ull ? ~0ull : (unsigned long long)need128;
    if (int rc = read_status(c)) return rc;         // (synchronises; iters_total as the device has it)
    size_t freeb = 0, totalb = 0;
    HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
    if (need > freeb)
        return fail(c, DOPF_E_NOMEM, "trace: the ring of %d slots of %llu bytes needs %llu bytes, the device has %llu free",
                    capacity, (unsigned long long)t.lay.slot_bytes, need, (unsigned long long)freeb);
    t.base = c->host_st.iters_total;
    TraceBlock hb;
    trace_fill_block(&hb, t.lay, v, t.base);
    c->trace = t;
    dopf_ctx::Trace &tr = c->trace;
    hipError_t e = hipMalloc((void **)&tr.ring, (size_t)capacity * t.lay.slot_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr.blk, sizeof(TraceBlock));
    if (e == hipSuccess && levels) e = hipMalloc((void **)&tr.level, (size_t)t.level_slots * v.S * v.T * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(tr.blk, &hb, sizeof hb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        trace_release(c);
        (void)hipGetLastError();
        return fail(c, e == hipErrorOutOfMemory ? DOPF_E_NOMEM : DOPF_E_DEVICE, "trace: allocating the ring of %d slots of %llu bytes (%llu bytes): %s",
                    capacity, (unsigned long long)t.lay.slot_bytes, need, hipGetErrorString(e));
    }
    tr.active = true;
    drop_graphs(c);             // the chain gains a launch: captured again at the next dopf_iterate
    return DOPF_OK;
}

int dopf_trace_end(dopf_ctx *c)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = trace_needs_active(c, "dopf_trace_end")) return rc;
    DeviceGuard guard(c->device);
    HIPCHK(c, hipStreamSynchronize(c->main));
    drop_graphs(c);             // the chain loses its last launch
    trace_release(c);
    return DOPF_OK;
}

int dopf_trace_reset(dopf_ctx *c)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = trace_needs_active(c, "dopf_trace_reset")) return rc;
    DeviceGuard guard(c->device);
    if (int rc = read_status(c)) return rc;
    // ordered on the context's stream; the graphs read base at this address (no capture again)
    c->trace.base = c->host_st.iters_total;
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&c->trace.blk->base), c->trace.base, 1, c->main));
    return DOPF_OK;
}

int dopf_trace_info(dopf_ctx *c, int32_t *what, int32_t *capacity, int32_t *held, int32_t *recorded)
{
    if (!c) return DOPF_E_INVALID;
    // (no trace: all zeros. recorded needs no read-back: dopf_iterate alone advances a traced context, and it ends with a status read)
    const dopf_ctx::Trace &t = c->trace;
    const int rec = t.active ? c->host_st.iters_total - t.base : 0;
    if (what) *what = t.what;
    if (capacity) *capacity = t.capacity;
    if (held) *held = t.active ? trace_held(rec, t.capacity) : 0;
    if (recorded) *recorded = rec;
    return DOPF_OK;
}

int dopf_trace_read(dopf_ctx *c, int32_t first, int32_t n, double *rows, int32_t *iteration, int32_t *converged,
                    double *lambda, double *mu, double *rho, double *injection, double *avg_U, double *avg_K, double *line_util,
                    double *P, double *D, double *C, double *E)
{
    if (!c) return DOPF_E_INVALID;
    if (int rc = trace_needs_active(c, "dopf_trace_read")) return rc;
    const dopf_ctx::Trace &t = c->trace;
    const DevView &v = c->v;
    const int rec = c->host_st.iters_total - t.base, held = trace_held(rec, t.capacity);
    if (first < 0 || n < 0 || (long long)first + n > held)
        return fail(c, DOPF_E_INVALID, "dopf_trace_read: slots [%d, %d) outside the %d held (recorded %d, capacity %d)", first, first + n, held,
                    rec, t.capacity);
    double *out[kTraceSections] = {lambda, mu, rho, injection, avg_U, avg_K, line_util, P, D, C};
    static const char *const names[kTraceSections] = {"lambda", "mu", "rho", "injection", "avg_U", "avg_K", "line_util", "P", "D", "C"};
    static const char *const bits[3] = {"DOPF_TRACE_DUALS", "DOPF_TRACE_CONSENSUS", "DOPF_TRACE_PRIMAL"};
    for (int k = 0; k < kTraceSections; ++k)
        if (out[k] && !(t.what & trace_bit_of(k)))
            return fail(c, DOPF_E_INVALID, "dopf_trace_read: %s is given, but the trace was begun without %s", names[k],
                        bits[trace_bit_of(k) == kTraceDuals ? 0 : trace_bit_of(k) == kTraceConsensus ? 1 : 2]);
    if (E && !(t.what & kTracePrimal))
        return fail(c, DOPF_E_INVALID, "dopf_trace_read: E is given, but the trace was begun without DOPF_TRACE_PRIMAL");
    if (n == 0) return DOPF_OK;
    DeviceGuard guard(c->device);
    const size_t sb = t.lay.slot_bytes, T = (size_t)v.T, ST = (size_t)v.S * T;
    const bool levels = E && v.S > 0;
    // whole slots come over in runs that are contiguous in the ring, on the context's stream behind what is queued there, a few MiB
    // at a time; the sections are taken apart here. With E: level_slots slots at a time, whose levels k_derive_level(_eff) forms
    // from the slot's D and C under the initial levels and efficiencies stored now.
    size_t batch = std::max<size_t>(1, ((size_t)8 << 20) / sb);
    if (levels) batch = std::min(batch, (size_t)t.level_slots);
    batch = std::min(batch, (size_t)n);
    std::vector<char> stage(batch * sb);
    std::vector<double> lev(levels ? batch * ST : 0);
    const int oldest = trace_oldest(rec, t.capacity);
    for (int done = 0; done < n;) {
        const int ring0 = (int)(((long long)oldest + first + done) % t.capacity);
        const int cnt = (int)std::min<size_t>(batch, (size_t)std::min(n - done, t.capacity - ring0));
        const char *src = t.ring + (size_t)ring0 * sb;
        HIPCHK(c, hipMemcpyAsync(stage.data(), src, (size_t)cnt * sb, hipMemcpyDeviceToHost, c->main));
        if (levels) {
            for (int j = 0; j < cnt; ++j) {
                DevView vs = v;
                vs.D = reinterpret_cast<double *>(const_cast<char *>(src) + (size_t)j * sb + t.lay.off[kSecD]);
                vs.C = reinterpret_cast<double *>(const_cast<char *>(src) + (size_t)j * sb + t.lay.off[kSecC]);
                vs.E = t.level + (size_t)j * ST;
                launch_derive_level(vs, c->plan, c->main);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(lev.data(), t.level, (size_t)cnt * ST * sizeof(double), hipMemcpyDeviceToHost, c->main));
        }
        HIPCHK(c, hipStreamSynchronize(c->main));
        for (int j = 0; j < cnt; ++j) {
            const char *slot = stage.data() + (size_t)j * sb;
            const size_t i = (size_t)done + j;
            TraceRow row;
            memcpy(&row, slot, sizeof row);
            if (rows) { memcpy(rows + 4 * i, row.res, 3 * sizeof(double)); rows[4 * i + 3] = row.total_cost; }
            if (iteration) iteration[i] = row.iteration;
            if (converged) converged[i] = row.converged;
            for (int k = 0; k < kTraceSections; ++k) {
                const size_t len = t.lay.n[k];
                if (!out[k] || len == 0) continue;
                const char *sec = slot + t.lay.off[k];
                if (k < kSecP) { memcpy(out[k] + len * i, sec, len * sizeof(double)); continue; }
                // device rows are in node-sorted order; hand them back in the caller's agent order
                const std::vector<int> &perm = k == kSecP ? c->gen_perm : c->sto_perm;
                for (size_t r = 0; r < perm.size(); ++r)
                    memcpy(out[k] + len * i + (size_t)perm[r] * T, sec + r * T * sizeof(double), T * sizeof(double));
            }
            if (levels)
                for (size_t r = 0; r < c->sto_perm.size(); ++r)
                    memcpy(E + ST * i + (size_t)c->sto_perm[r] * T, lev.data() + (size_t)j * ST + r * T, T * sizeof(double));
        }
        done += cnt;
    }
    return DOPF_OK;
}

int dopf_debug_stats(dopf_ctx *c, uint64_t *out3 /* 15 values */)
{
    if (!c || !out3) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    int rc = read_status(c);
    if (rc) return rc;
    out3[0] = c->host_st.dbg_scans; out3[1] = c->host_st.dbg_wave_loops; out3[2] = c->host_st.dbg_events;
    {   // warm-start kernel, LAST iteration: storages it solved / left to the scan kernel
        std::vector<int> f(c->v.nStoItems);
        if (!f.empty()) HIPCHK(c, hipMemcpy(f.data(), c->v.item_fail, f.size() * sizeof(int), hipMemcpyDeviceToHost));
        uint64_t nf = 0;
        for (int x : f) nf += (uint64_t)x;
        out3[4] = c->v.use_warm ? nf : (uint64_t)c->v.S;
        out3[3] = (uint64_t)c->v.S - out3[4];
    }
    for (int i = 0; i < 4; ++i) out3[5 + i] = c->host_st.dbg_reason[i];
    for (int i = 0; i < 6; ++i) out3[9 + i] = c->host_st.dbg_cyc[i];
    return DOPF_OK;
}

int dopf_debug_quiet(dopf_ctx *c, int64_t *out3)
{
    if (!c || !out3) return DOPF_E_INVALID;
    // (a context on a communicator: the chain without k_reduce on a peer exchange, DevView::slackGlobal)
    out3[0] = quiet_allowed(c) ? 1 : 0;
    out3[1] = c->quiet ? 1 : 0; out3[2] = (int64_t)c->quiet_parked;
    return DOPF_OK;
}

int dopf_debug_timeline(dopf_ctx *c, uint64_t *out, int32_t n)
{
    if (!c || !out) return DOPF_E_INVALID;
    DeviceGuard guard(c->device);
    hipStreamSynchronize(c->main);
    return debug_timeline((unsigned long long *)out, n);
}

int64_t dopf_solver_failures(dopf_ctx *c)
{
    if (!c) return -1;
    DeviceGuard guard(c->device);
    if (read_status(c)) return -1;
    return (int64_t)c->host_st.solver_fail;
}

}  // extern "C"
