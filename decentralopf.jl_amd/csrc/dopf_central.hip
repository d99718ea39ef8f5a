// dopf_central.hip — host side of the central reference (dopf_central_solve, include/dopf.h).
//
// Replaces src/opf_central_reference.jl:1-81: sets the LP up from the same dopf_problem the decentral path takes, runs the
// primal-dual iteration of kernels_central.hip in batches, looks at the primal / dual objectives and the worst constraint
// violation of the last iterate and of the running average between batches, restarts from the better one when its
// normalised gap has halved, stops at the requested tolerance.
//
// dopf_central_solve_ex: the LP with initial levels, terminal bands and availability profiles. Only boxes and right-hand sides change,
// so the step sizes, the averaging and the restarts below are untouched. The inputs go through the ADMM path's own setters on the
// temporary context (their checks, their codes, their device arrays); Plan::genAvail / stoLV then select the sweeps' instantiations.
//
// dopf_central_solve_lossy: the same with storage efficiencies (DOPF_F_STO_EFFICIENCY on the temporary context, stoLV 3). The level
// rows' coefficients change, and with them the storages' gradient, step sizes and levels — all inside kc_sto<., 3>, which reads
// sto_eff_alpha(v) / sto_eff_beta(v). The balance and flow rows act on the injection D - C, whose coefficients stay, so the step-size
// block below (tauN, sigB, sigF) is that of the lossless LP. dopf_central_solve_ex is this entry without efficiencies.
//
// dopf_central_solve_coupled: the same with generator ramp limits, an anchor, energy budgets and a line-rating table. The
// rating table goes through DOPF_F_LINE_RATING and dopf_set_line_rating on the temporary context (kc_dual<., true> reads it). The ramp
// and budget arrays are checked by the setters' own checks (check_generator_ramp_values, check_generator_energy_budget_values) and
// kept in allocations of this solve, in the context's sorted generator order: the temporary context has neither flag — the ADMM
// kernels' scratch behind gen_pmax is nothing the LP needs, and the two never go together there. With any of the five arrays given
// kc_gen_rows runs in kc_gen's place; its rows have multipliers (yR, yQ), running sums and restart copies like the others.
//
// Long horizons: every entry takes any T. Where a row couples timesteps — storages, ramps, budgets — beyond the one-wave
// sweeps' horizon, the entry sets DOPF_F_LONG_HORIZON on the temporary context itself (what counts is the shape, as with the other
// inputs), and kc_sto_long / kc_gen_rows_long run in kc_sto's / kc_gen_rows' place. The iteration around them is the same.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "dopf_ctx.h"

using namespace dopf;

namespace {

template <class Tp>
int calloc_dev(dopf_ctx *c, Tp **out, size_t n)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(Tp);
    HIPCHK(c, hipMalloc(&p, bytes));
    c->allocs.push_back(p);                 // freed by dopf_destroy
    // (the context's stream does not synchronise with the null stream: the blocking copies that fill some of these arrays
    // must not overtake the zeroing — wait for it here)
    HIPCHK(c, hipMemsetAsync(p, 0, bytes, c->main));
    HIPCHK(c, hipStreamSynchronize(c->main));
    *out = (Tp *)p;
    return DOPF_OK;
}

struct Metrics {
    double pobj, dobj, pinf, gap;
};

// what dopf_central_solve_coupled takes and returns beyond dopf_central_solve_lossy (all null: that entry's body, its bits)
struct Coupling {
    const double *rating, *ramp_up, *ramp_down, *prev, *e_min, *e_max;
    double *ramp_dual, *budget_dual;
    bool rows() const { return ramp_up || ramp_down || prev || e_min || e_max; }
};

}  // namespace

extern "C" int dopf_central_solve(const dopf_problem *p, const dopf_params *q, double tol, int32_t max_iters,
                                  dopf_central_result *res, double *P, double *D, double *C, double *E,
                                  double *system_price, double *nodal_price, double *line_utilization,
                                  double *flow_upper_dual, double *flow_lower_dual)
{
    return dopf_central_solve_ex(p, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr, tol, max_iters, res, P, D, C, E,
                                 system_price, nodal_price, line_utilization, flow_upper_dual, flow_lower_dual);
}

namespace {

// the body of dopf_central_solve_ex / dopf_central_solve_lossy; entry: the name a refusal's message carries
int central_solve_impl(const char *entry, const dopf_problem *p, const dopf_params *q, const double *sto_e0_in,
                       const double *sto_end_lo_in, const double *sto_end_hi_in, const double *sto_eta_c_in, const double *sto_eta_d_in,
                       int32_t n_profiles, const double *profiles, const int32_t *profile_of, const Coupling &cp,
                       double tol, int32_t max_iters,
                       dopf_central_result *res, double *P, double *D, double *C, double *E,
                       double *system_price, double *nodal_price, double *line_utilization,
                       double *flow_upper_dual, double *flow_lower_dual);

}  // namespace

extern "C" int dopf_central_solve_ex(const dopf_problem *p, const dopf_params *q, const double *sto_e0_in,
                                     const double *sto_end_lo_in, const double *sto_end_hi_in,
                                     int32_t n_profiles, const double *profiles, const int32_t *profile_of,
                                     double tol, int32_t max_iters,
                                     dopf_central_result *res, double *P, double *D, double *C, double *E,
                                     double *system_price, double *nodal_price, double *line_utilization,
                                     double *flow_upper_dual, double *flow_lower_dual)
{
    return central_solve_impl("dopf_central_solve_ex", p, q, sto_e0_in, sto_end_lo_in, sto_end_hi_in, nullptr, nullptr, n_profiles, profiles,
                              profile_of, Coupling{}, tol, max_iters, res, P, D, C, E, system_price, nodal_price, line_utilization, flow_upper_dual,
                              flow_lower_dual);
}

extern "C" int dopf_central_solve_lossy(const dopf_problem *p, const dopf_params *q, const double *sto_e0_in,
                                        const double *sto_end_lo_in, const double *sto_end_hi_in,
                                        const double *sto_eta_c_in, const double *sto_eta_d_in,
                                        int32_t n_profiles, const double *profiles, const int32_t *profile_of,
                                        double tol, int32_t max_iters,
                                        dopf_central_result *res, double *P, double *D, double *C, double *E,
                                        double *system_price, double *nodal_price, double *line_utilization,
                                        double *flow_upper_dual, double *flow_lower_dual)
{
    return central_solve_impl("dopf_central_solve_lossy", p, q, sto_e0_in, sto_end_lo_in, sto_end_hi_in, sto_eta_c_in, sto_eta_d_in, n_profiles,
                              profiles, profile_of, Coupling{}, tol, max_iters, res, P, D, C, E, system_price, nodal_price, line_utilization,
                              flow_upper_dual, flow_lower_dual);
}

extern "C" int dopf_central_solve_coupled(const dopf_problem *p, const dopf_params *q, const double *sto_e0_in,
                                          const double *sto_end_lo_in, const double *sto_end_hi_in,
                                          const double *sto_eta_c_in, const double *sto_eta_d_in,
                                          int32_t n_profiles, const double *profiles, const int32_t *profile_of,
                                          const double *line_rating, const double *gen_ramp_up, const double *gen_ramp_down,
                                          const double *gen_prev, const double *gen_e_min, const double *gen_e_max,
                                          double tol, int32_t max_iters,
                                          dopf_central_result *res, double *P, double *D, double *C, double *E,
                                          double *system_price, double *nodal_price, double *line_utilization,
                                          double *flow_upper_dual, double *flow_lower_dual, double *ramp_dual, double *budget_dual)
{
    // the checks that need no values come first: they are seen without a device
    static const char *const entry = "dopf_central_solve_coupled";
    if (!gen_ramp_up != !gen_ramp_down) return fail(nullptr, DOPF_E_INVALID, "%s: ramp_up and ramp_down must both be given or both be NULL", entry);
    if (!(tol > 0)) return fail(nullptr, DOPF_E_INVALID, "%s: tol = %g (> 0 wanted)", entry, tol);
    if (max_iters < 1) return fail(nullptr, DOPF_E_INVALID, "%s: max_iters = %d (>= 1 wanted)", entry, max_iters);
    const Coupling cp{line_rating, gen_ramp_up, gen_ramp_down, gen_prev, gen_e_min, gen_e_max, ramp_dual, budget_dual};
    return central_solve_impl(entry, p, q, sto_e0_in, sto_end_lo_in, sto_end_hi_in, sto_eta_c_in, sto_eta_d_in, n_profiles, profiles, profile_of,
                              cp, tol, max_iters, res, P, D, C, E, system_price, nodal_price, line_utilization, flow_upper_dual, flow_lower_dual);
}

namespace {

int central_solve_impl(const char *entry, const dopf_problem *p, const dopf_params *q, const double *sto_e0_in,
                       const double *sto_end_lo_in, const double *sto_end_hi_in, const double *sto_eta_c_in, const double *sto_eta_d_in,
                       int32_t n_profiles, const double *profiles, const int32_t *profile_of, const Coupling &cp,
                       double tol, int32_t max_iters,
                       dopf_central_result *res, double *P, double *D, double *C, double *E,
                       double *system_price, double *nodal_price, double *line_utilization,
                       double *flow_upper_dual, double *flow_lower_dual)
{
    if (!p || !q || !res || !(tol > 0) || max_iters < 1) return fail(nullptr, DOPF_E_INVALID, "bad argument");
    memset(res, 0, sizeof *res);
    const bool has_rows = cp.rows() && p->G > 0, has_rating = cp.rating && p->L > 0;
    dopf_ctx *c = nullptr;
    dopf_params qq = *q;
    qq.stream = nullptr;
    qq.flags &= ~(DOPF_F_OVERLAP_AGENTS | DOPF_F_STO_EFFICIENCY);     // (the caller's efficiency flag is ignored: lossless unless the arrays are given)
    // the LP takes no ramps: a network context's two ramp flags (bit 31 is the word's sign bit: masked as a number) would only cost
    // k_gen_ramp_net's scratch — and DOPF_F_GEN_RAMP_NETWORK alone is nothing dopf_create accepts
    qq.flags &= 0x7fffffff;
    if (p->L > 0) qq.flags &= ~DOPF_F_GEN_RAMP;
    // every input that is given sets its flag (the caller's own flags stay: a flag without its input is that feature's default)
    const bool has_e0 = sto_e0_in != nullptr, has_band = sto_end_lo_in || sto_end_hi_in;
    const bool has_avail = n_profiles != 0 || profiles || profile_of;
    const bool has_eta = sto_eta_c_in || sto_eta_d_in;
    if (has_eta) qq.flags |= DOPF_F_STO_EFFICIENCY;
    if (has_e0) qq.flags |= DOPF_F_STO_INITIAL_LEVEL;
    if (has_band) qq.flags |= DOPF_F_STO_TERMINAL_LEVEL;
    if (has_avail) qq.flags |= DOPF_F_GEN_AVAILABILITY;
    if (has_rating) qq.flags |= DOPF_F_LINE_RATING;
    // ... and so does the shape: a row that couples timesteps beyond one wave's horizon runs on the long sweeps (kc_sto_long through
    // the context's Plan::stoLong, kc_gen_rows_long through cv.longRows). The caller's DOPF_F_LONG_HORIZON is neither needed nor harmful
    const bool long_horizon = p->T > kCentralWaveHorizon;
    if (long_horizon && (p->S > 0 || has_rows)) qq.flags |= DOPF_F_LONG_HORIZON;
    int rc = dopf_create(&c, p, &qq);       // sorted agents, items, node maps, partial-sum arrays, P/D/C/E (zero)
    if (rc) return rc;
    // (callers read dopf_last_error(NULL): the temporary context's message has to outlive it)
    struct Guard { dopf_ctx *c; ~Guard() { keep_error(c); dopf_destroy(c); } } guard{c};
    DeviceGuard dev(c->device);
    {   // the efficiencies first (the level setters then check reachability under them), then e0 (the band's reachability is
        // checked from it), then the band, then the profiles; a refusal is the setter's code, and its message names this entry
        rc = DOPF_OK;
        if (has_eta) rc = dopf_set_storage_efficiency(c, sto_eta_c_in, sto_eta_d_in);
        if (!rc && has_e0) rc = dopf_set_storage_initial_level(c, sto_e0_in);
        if (!rc && has_band) rc = dopf_set_storage_terminal_level(c, sto_end_lo_in, sto_end_hi_in);
        if (!rc && has_avail) rc = dopf_set_generator_availability(c, n_profiles, profiles, profile_of);
        if (!rc && has_rating) rc = dopf_set_line_rating(c, cp.rating);
        if (rc) {
            const std::string why = c->err;
            return fail(c, rc, "%s: %s", entry, why.c_str());
        }
    }
    const DevView &v = c->v;
    const int N = v.N, L = v.L, T = v.T, G = v.G, S = v.S;
    const size_t NT = (size_t)N * T, LT = (size_t)L * T, GT = (size_t)G * T, ST = (size_t)S * T;

    CentralView cv{};
    cv.v = v;
    cv.rated = has_rating ? 1 : 0;
    cv.longRows = (long_horizon || (q->flags & DOPF_F_DEBUG_LONG_STO)) ? 1 : 0;
    if (has_rows) {
        // the ramps, the anchor and the budgets: the setters' checks under the availability table of this call (the context's profile
        // indices refer to the caller's table), then the five arrays in the context's sorted order — the map dopf_get_primal uses
        std::vector<double> pm(G), h(5 * (size_t)G);
        for (int i = 0; i < G; ++i) pm[i] = p->gen_pmax[c->gen_perm[i]];
        if ((rc = check_generator_ramp_values(c, entry, pm.data(), profiles, cp.ramp_up, cp.ramp_down, cp.prev))) return rc;
        if ((rc = check_generator_energy_budget_values(c, entry, pm.data(), profiles, cp.e_min, cp.e_max))) return rc;
        for (int i = 0; i < G; ++i) {
            const int a = c->gen_perm[i];
            h[i] = cp.ramp_up ? cp.ramp_up[a] + 0.0 : INFINITY;
            h[(size_t)G + i] = cp.ramp_down ? cp.ramp_down[a] + 0.0 : INFINITY;
            h[2 * (size_t)G + i] = cp.prev ? cp.prev[a] + 0.0 : std::nan("");
            h[3 * (size_t)G + i] = cp.e_min ? cp.e_min[a] + 0.0 : 0.0;
            h[4 * (size_t)G + i] = cp.e_max ? cp.e_max[a] + 0.0 : INFINITY;
        }
        double *d = nullptr;
        if ((rc = calloc_dev(c, &d, h.size()))) return rc;
        HIPCHK(c, hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        cv.rows_in = d;
        if ((rc = calloc_dev(c, &cv.yR, GT)) || (rc = calloc_dev(c, &cv.aR, GT)) || (rc = calloc_dev(c, &cv.yQ, G)) ||
            (rc = calloc_dev(c, &cv.aQ, G)) || (rc = calloc_dev(c, &cv.m_rows, 3 * (size_t)v.nGenItems))) return rc;
    }
    cv.w = 1.0;
    cv.sigB = 1.0 / std::max(1, G + 2 * S);
    {   // diagonal step sizes (Pock & Chambolle, alpha = 1): column / row sums of |K|
        std::vector<double> absH(N, 0.0), tauN(N), sigF(L, 0.0);
        std::vector<int> gb(N + 1), sb(N + 1);
        HIPCHK(c, hipMemcpy(gb.data(), v.node_gen_beg, sizeof(int) * (N + 1), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(sb.data(), v.node_sto_beg, sizeof(int) * (N + 1), hipMemcpyDeviceToHost));
        for (int n = 0; n < N; ++n) {
            for (int l = 0; l < L; ++l) absH[n] += std::fabs(p->ptdf[l + (size_t)L * n]);
            tauN[n] = 1.0 / (1.0 + absH[n]);
        }
        for (int l = 0; l < L; ++l) {
            double rs = 0.0;
            for (int n = 0; n < N; ++n) rs += std::fabs(p->ptdf[l + (size_t)L * n]) * ((gb[n + 1] - gb[n]) + 2.0 * (sb[n + 1] - sb[n]));
            sigF[l] = 1.0 / std::max(rs, 1e-300);
        }
        double *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
        if ((rc = calloc_dev(c, &d1, N)) || (rc = calloc_dev(c, &d2, N)) || (rc = calloc_dev(c, &d3, L))) return rc;
        HIPCHK(c, hipMemcpy(d1, tauN.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d2, absH.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        if (L) HIPCHK(c, hipMemcpy(d3, sigF.data(), sizeof(double) * L, hipMemcpyHostToDevice));
        cv.tauN = d1; cv.absHn = d2; cv.sigF = d3;
    }
    if ((rc = calloc_dev(c, &cv.yb, T)) || (rc = calloc_dev(c, &cv.yf, LT)) || (rc = calloc_dev(c, &cv.yE, ST)) ||
        (rc = calloc_dev(c, &cv.aP, GT)) || (rc = calloc_dev(c, &cv.aD, ST)) || (rc = calloc_dev(c, &cv.aC, ST)) ||
        (rc = calloc_dev(c, &cv.aE, ST)) || (rc = calloc_dev(c, &cv.ab, T)) || (rc = calloc_dev(c, &cv.af, LT)) ||
        (rc = calloc_dev(c, &cv.pi, NT)) || (rc = calloc_dev(c, &cv.m_gen, v.nGenItems)) ||
        (rc = calloc_dev(c, &cv.m_sto, 3 * (size_t)v.nStoItems)) || (rc = calloc_dev(c, &cv.m_dual, 3 * (size_t)T)))
        return rc;
    DevView vred = v;                        // k_reduce without the slack-sum part: nodal sums and the cost only
    vred.L = 0;
    vred.sliceDual = 0;
    vred.part_T = nullptr;                   // (kc_gen / kc_sto write partial rows, [row][t])
    vred.genRows = 0;                        // (kc_gen writes one partial row per item)

    // (per generator item: kc_gen's reduced-cost term, or kc_gen_rows' three)
    std::vector<double> mg((has_rows ? 3 : 1) * (size_t)v.nGenItems), ms(3 * (size_t)v.nStoItems), md(3 * (size_t)T);
    double dmax = 0.0;
    for (size_t i = 0; i < NT; ++i) dmax = std::max(dmax, std::fabs(p->demand[i]));
    auto metrics = [&](const double *XP, const double *XD, const double *XC, const double *XE, const double *yb, const double *yf,
                       const double *XR, const double *XQ, double scale, Metrics &m) -> int {
        central_launch_metrics(cv, c->plan, vred, XP, XD, XC, XE, yb, yf, XR, XQ, scale, c->main);
        double cost = 0.0;
        HIPCHK(c, hipMemcpyAsync(&cost, v.cons + NT, sizeof(double), hipMemcpyDeviceToHost, c->main));
        if (!mg.empty()) HIPCHK(c, hipMemcpyAsync(mg.data(), has_rows ? cv.m_rows : cv.m_gen, mg.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
        if (!ms.empty()) HIPCHK(c, hipMemcpyAsync(ms.data(), cv.m_sto, ms.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
        HIPCHK(c, hipMemcpyAsync(md.data(), cv.m_dual, md.size() * sizeof(double), hipMemcpyDeviceToHost, c->main));
        HIPCHK(c, hipStreamSynchronize(c->main));
        double d = 0.0, inf = 0.0;
        if (has_rows) for (size_t i = 0; i < mg.size(); i += 3) { d += mg[i] + mg[i + 1]; inf = std::max(inf, mg[i + 2]); }
        else for (double x : mg) d += x;
        for (size_t i = 0; i < ms.size(); i += 3) { d += ms[i] - ms[i + 2]; inf = std::max(inf, ms[i + 1]); }
        for (size_t t = 0; t < (size_t)T; ++t) { inf = std::max(inf, std::max(md[3 * t], md[3 * t + 1])); d += md[3 * t + 2]; }
        m.pobj = cost; m.dobj = d; m.pinf = std::max(inf, 0.0);
        m.gap = std::fabs(cost - d) / (1.0 + std::fabs(cost)) + m.pinf / (1.0 + dmax);
        return DOPF_OK;
    };

    // dopf_central_solve_coupled with any of its inputs: the primal weight follows the iterates (PDLP's update). At every restart
    // w <- sqrt(w |dy| / |dx|) with dx, dy the primal and dual points' moves since the last restart, so that the step sizes balance
    // the two distances still to go. With w = 1 throughout, the network case with ramps, anchors and budgets stalled at a gap of
    // 2.3e-7 from iteration 60 000 to 200 000. The older entries keep w = 1, and with it their bits.
    const bool adapt_w = has_rows || has_rating;
    struct Anchored { double *cur, *anchor; size_t n; bool primal; };
    std::vector<Anchored> moved;
    double *diff_part = nullptr;
    if (adapt_w) {
        for (auto pr : {Anchored{v.P, nullptr, GT, true}, Anchored{v.D, nullptr, ST, true}, Anchored{v.C, nullptr, ST, true},
                        Anchored{cv.yb, nullptr, (size_t)T, false}, Anchored{cv.yf, nullptr, LT, false}, Anchored{cv.yE, nullptr, ST, false},
                        Anchored{cv.yR, nullptr, has_rows ? GT : 0, false}, Anchored{cv.yQ, nullptr, has_rows ? (size_t)G : 0, false}}) {
            if (!pr.n) continue;
            if ((rc = calloc_dev(c, &pr.anchor, pr.n))) return rc;          // (zeros: the starting point)
            moved.push_back(pr);
        }
        if ((rc = calloc_dev(c, &diff_part, kCentralDiffBlocks))) return rc;
    }
    auto update_weight = [&]() -> int {
        double d2[2] = {0.0, 0.0};           // dual, primal
        std::vector<double> part(kCentralDiffBlocks);
        for (const Anchored &a : moved) {
            const int nb = central_diff_blocks(a.n);
            central_launch_diff_sq(a.cur, a.anchor, a.n, diff_part, c->main);
            HIPCHK(c, hipMemcpyAsync(part.data(), diff_part, nb * sizeof(double), hipMemcpyDeviceToHost, c->main));
            HIPCHK(c, hipStreamSynchronize(c->main));
            for (int i = 0; i < nb; ++i) d2[a.primal] += part[i];
            HIPCHK(c, hipMemcpyAsync(a.anchor, a.cur, a.n * sizeof(double), hipMemcpyDeviceToDevice, c->main));
        }
        const double dx = std::sqrt(d2[1]), dy = std::sqrt(d2[0]);
        if (dx > 1e-10 && dy > 1e-10) cv.w = std::exp(0.5 * std::log(dy / dx) + 0.5 * std::log(cv.w));
        return DOPF_OK;
    };
    const int batch = 200, max_avg = 4000;
    int it = 0, navg = 0;
    double last_gap = INFINITY;
    Metrics mc{}, ma{};
    bool use_avg = false, done = false;
    while (it < max_iters && !done) {
        const int nb = std::min(batch, max_iters - it);
        for (int k = 0; k < nb; ++k) central_launch_iteration(cv, c->plan, vred, c->main);
        HIPCHK(c, hipGetLastError());
        it += nb; navg += nb;
        if ((rc = metrics(v.P, v.D, v.C, cv.yE, cv.yb, cv.yf, cv.yR, cv.yQ, 1.0, mc))) return rc;
        if ((rc = metrics(cv.aP, cv.aD, cv.aC, cv.aE, cv.ab, cv.af, cv.aR, cv.aQ, 1.0 / navg, ma))) return rc;
        use_avg = ma.gap < mc.gap;
        const Metrics &best = use_avg ? ma : mc;
        done = best.gap <= tol;
        if (done || best.gap < 0.5 * last_gap || navg >= max_avg) {
            if (use_avg) {                  // restart from the average
                const double sc = 1.0 / navg;
                central_launch_scale_copy_primal(cv, c->plan, sc, c->main);      // (P, D, C: kept inside their boxes)
                central_launch_scale_copy(cv.yE, cv.aE, sc, ST, c->main);
                central_launch_scale_copy(cv.yb, cv.ab, sc, T, c->main);
                central_launch_scale_copy(cv.yf, cv.af, sc, LT, c->main);
                if (has_rows) {
                    central_launch_scale_copy(cv.yR, cv.aR, sc, GT, c->main);
                    central_launch_scale_copy(cv.yQ, cv.aQ, sc, G, c->main);
                }
            }
            last_gap = best.gap;
            if (adapt_w && (rc = update_weight())) return rc;
            for (auto pr : {std::make_pair(cv.aP, GT), std::make_pair(cv.aD, ST), std::make_pair(cv.aC, ST), std::make_pair(cv.aE, ST),
                            std::make_pair(cv.ab, (size_t)T), std::make_pair(cv.af, LT), std::make_pair(cv.aR, has_rows ? GT : 0),
                            std::make_pair(cv.aQ, has_rows ? (size_t)G : 0)})
                if (pr.second) HIPCHK(c, hipMemsetAsync(pr.first, 0, pr.second * sizeof(double), c->main));
            navg = 0;
        }
    }
    // the accepted point is in v.P / v.D / v.C, (yb, yf, yE); its levels, injections and flows come from one more metrics pass
    Metrics mf{};
    if ((rc = metrics(v.P, v.D, v.C, cv.yE, cv.yb, cv.yf, cv.yR, cv.yQ, 1.0, mf))) return rc;
    res->objective = mf.pobj; res->dual_objective = mf.dobj; res->primal_infeasibility = mf.pinf; res->gap = mf.gap;
    res->iterations = it; res->converged = mf.gap <= tol ? 1 : 0;
    c->level_from_primal = false;            // (the metrics pass has written the accepted point's levels into v.E)
    if ((rc = dopf_get_primal(c, P, D, C, E))) return rc;
    std::vector<double> yb(T), yf(LT);
    HIPCHK(c, hipMemcpy(yb.data(), cv.yb, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (LT) HIPCHK(c, hipMemcpy(yf.data(), cv.yf, sizeof(double) * LT, hipMemcpyDeviceToHost));
    if (system_price) for (int t = 0; t < T; ++t) system_price[t] = -yb[t];                  // dual.(EB), opf_central_reference.jl:66
    if (nodal_price) {
        // the reference's formula (:71-79): lambda + sum_l (dual FlowUpper + dual FlowLower)[l,t] ptdf[l,n]. Both duals are
        // d objective / d f_max <= 0, i.e. -|yf| whichever limit binds (this is what the script prints; the marginal price
        // of an injection would carry the lower limit's dual with the opposite sign)
        for (int t = 0; t < T; ++t)
            for (int n = 0; n < N; ++n) {
                double pr = -yb[t];
                for (int l = 0; l < L; ++l) pr -= std::fabs(yf[l + (size_t)L * t]) * p->ptdf[l + (size_t)L * n];
                nodal_price[n + (size_t)N * t] = pr;
            }
    }
    if (line_utilization && LT) HIPCHK(c, hipMemcpy(line_utilization, v.flow, sizeof(double) * LT, hipMemcpyDeviceToHost));
    // dual.(FlowUpper), dual.(FlowLower) (:71): the multiplier of |flow| <= max_capacity is positive where the upper limit
    // binds and negative where the lower one does; either dual is d objective / d max_capacity <= 0
    for (size_t i = 0; i < LT; ++i) {
        if (flow_upper_dual) flow_upper_dual[i] = -std::max(yf[i], 0.0);
        if (flow_lower_dual) flow_lower_dual[i] = -std::max(-yf[i], 0.0);
    }
    // the ramp and budget rows' duals, d objective / d right-hand side like the others: negative where the row's upper end binds
    // (more room there lowers the cost), positive where the lower end does; 0 for a generator without the row
    if (cp.ramp_dual) {
        std::vector<double> y(GT, 0.0);
        if (has_rows && GT) HIPCHK(c, hipMemcpy(y.data(), cv.yR, sizeof(double) * GT, hipMemcpyDeviceToHost));
        for (int i = 0; i < G; ++i)
            for (int t = 0; t < T; ++t) cp.ramp_dual[t + (size_t)T * c->gen_perm[i]] = 0.0 - y[t + (size_t)T * i];
    }
    if (cp.budget_dual) {
        std::vector<double> y(G, 0.0);
        if (has_rows) HIPCHK(c, hipMemcpy(y.data(), cv.yQ, sizeof(double) * G, hipMemcpyDeviceToHost));
        for (int i = 0; i < G; ++i) cp.budget_dual[c->gen_perm[i]] = 0.0 - y[i];
    }
    return DOPF_OK;
}

}  // namespace
