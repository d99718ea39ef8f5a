// kernels_central.hip — the central reference on the device (gfx950, fp64).
//
// Replaces src/opf_central_reference.jl:16-57 (one JuMP model of the whole multi-period DC-OPF handed to Gurobi): the same
// LP solved by a first-order primal-dual method whose every step is the kind of work the decentral kernels do — a
// sweep over the agents' time series, the nodal sums, one PTDF product — so it runs on the same data layout and reuses
// k_reduce. It is the parity target of the decentral run ("converged objective within 1e-3 of the central optimum") for
// cases no LP solver on the host can take, and an algorithm independent of the ADMM iteration.
//
//   variables   x = (P[g,t], D[s,t], C[s,t]) in their boxes           (E is eliminated: E[s,t] = sum_{tau <= t} (C - D))
//   rows        balance_t:  sum_n I[n,t] = 0                           multiplier yb[t]   (free)
//               flows:      -f_max <= (ptdf I)[l,t] <= f_max           multiplier yf[l,t] (sign = which limit binds)
//               levels:     0 <= E[s,t] <= e_max                       multiplier yE[s,t]
//   PDHG        x+ = clamp(x - tau (c + K'y)),  y+ = prox(y + sigma K(2x+ - x))   with the diagonal step sizes of Pock &
//               Chambolle (tau_j = 1 / sum_i |K_ij|, sigma_i = 1 / sum_j |K_ij|), running averages and restarts to the better
//               of (last iterate, average) whenever its normalised gap has halved (the scheme of PDLP, without its line
//               search). Prototype and convergence record: scripts/proto_pdlp.py (machine precision in 4k-12k iterations on
//               config1, config2/10 and a 118-node case).
//   inputs      dopf_central_solve_ex (DOPF_F_STO_INITIAL_LEVEL, _TERMINAL_LEVEL, DOPF_F_GEN_AVAILABILITY): boxes and right-hand sides only,
//               K stays — box 0 <= P[g,t] <= cap[g,t] = gen_pmax[g] * f[prof[g]][t] (kc_gen<., AV>); level rows
//               lb_t - e0 <= sum_{tau <= t} (C - D) <= ub_t - e0 with [lb_t, ub_t] = [0, e_max], [lo, hi] at t = T-1 (kc_sto<., LV>).
//               Read from the arrays the ADMM kernels read: gen_prof(v), gen_avail_slot(v), sto_e0(v), sto_end_lo/hi(v).
//               dopf_central_solve_lossy (DOPF_F_STO_EFFICIENCY): the level rows become lb_t - e0 <= sum_{tau <= t} (be C - al D) <= ub_t - e0,
//               be = eta_c, al = 1 / eta_d from sto_eff_beta(v), sto_eff_alpha(v) — K itself changes, in the storages' columns only
//               (kc_sto<., 3>); the injection D - C, and with it the balance and flow rows, stay.
//               dopf_central_solve_coupled: more rows — ramp rows -rd <= P[g,t] - P[g,t-1] <= ru (t = 0: against an anchor) with
//               multipliers yR[g,t], budget rows e_min <= sum_t P[g,t] <= e_max with yQ[g] (kc_gen_rows in kc_gen's place;
//               central_rows.h) — and the flow rows' limits from a rating table (kc_dual<., true>).
//   horizons    kc_sto and kc_gen_rows hold a row in one wave's registers: T <= 512. Beyond it (every entry, no flag to set) kc_sto_long
//               and kc_gen_rows_long walk a row in tiles of 2048 timesteps with a whole block (central_long.h).
//   one text    A one-wave sweep and its long twin differ in who owns which timestep, how a neighbour's value arrives (a shuffle; LDS
//               and a tile carry) and how the item's sums are kept (a per-lane acc[]; part[t]). Everything else exists once: the level
//               rows' arithmetic in central_sto.h and the generator rows' in central_rows.h (plain C++, pinned on the CPU), a slot's
//               loads, stores and metrics in sto_primal_slot / sto_level_slot and gen_column_slot / gen_ramp_slot / gen_budget_row,
//               the reductions in block_tree_sum / block_tree_max, block_metrics and item_sums_store.
//   outputs     objective, P, D, C, E; system price = -yb (dual(EB) of the reference), nodal price = -(yb + ptdf' yf)
//               (src/opf_central_reference.jl:66-79).
#include <algorithm>

#include "central_long.h"
#include "central_sto.h"
#include "dopf_internal.h"

namespace dopf {

constexpr int KMAX = 8;                     // timesteps per lane in the one-wave sweeps (kc_sto, kc_gen_rows)
static_assert(kCentralWaveHorizon == 64 * KMAX, "dopf_central.hip switches to the long sweeps where a wave's registers end");
static_assert(kClSlots == 8, "the long sweeps' slot loops and the hand-over of yR[t+1] are written for 8 slots per thread");

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ double wave_prefix(double x, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// sum / maximum of x over the block's NT threads through red[NT], pairs at strides NT/2, NT/4, ... 1; the same bits in every thread.
// again: red is written again after the call (one more barrier).
template <int NT>
__device__ __forceinline__ double block_tree_sum(double *red, int tid, double x, bool again)
{
    red[tid] = x;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double r = red[0];
    if (again) __syncthreads();
    return r;
}

template <int NT>
__device__ __forceinline__ double block_tree_max(double *red, int tid, double x, bool again)
{
    red[tid] = x;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) { if (tid < s) red[tid] = fmax(red[tid], red[tid + s]); __syncthreads(); }
    const double r = red[0];
    if (again) __syncthreads();
    return r;
}

// the !ITER tail of the four row sweeps: four per-thread values over the block's four waves in a fixed order (an xor reduction in the
// wave, then (w0 + w1) + (w2 + w3) by thread 0), value MAXI a maximum and the others sums. On return thread 0 holds the block's four.
template <int MAXI>
__device__ __forceinline__ void block_metrics(double (&m)[4], double (*redm)[4], int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double o = __shfl_xor(m[i], d);
            m[i] = i == MAXI ? fmax(m[i], o) : m[i] + o;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) redm[wv][i] = m[i];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            m[i] = i == MAXI ? fmax(fmax(redm[0][i], redm[1][i]), fmax(redm[2][i], redm[3][i]))
                             : (redm[0][i] + redm[1][i]) + (redm[2][i] + redm[3][i]);
    }
}

// the one-wave sweeps' item sums: part[item][t] (part: v.part_sinj or v.part_ginj) = the four waves' acc of timestep t, added in a fixed
// order (lane ln's slot k is t = ln K + k)
__device__ __forceinline__ void item_sums_store(const double (&acc)[KMAX], double (*red)[64 * KMAX], double *part, int K, int T, int tid, int lane,
                                                int wv)
{
#pragma unroll
    for (int k = 0; k < KMAX; ++k) red[wv][lane * KMAX + k] = acc[k];
    __syncthreads();
    for (int i = tid; i < 64 * KMAX; i += 256) {
        const int ln = i / KMAX, k = i - ln * KMAX, t = ln * K + k;
        if (k < K && t < T) part[(size_t)blockIdx.x * T + t] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// pi[n,t] = yb[t] + sum_l ptdf[l,n] yf[l,t]   (the column of K' every unit at node n sees), candidate = scale * (yb, yf)
__global__ __launch_bounds__(256) void kc_price(CentralView c, const double *yb, const double *yf, double scale)
{
    extern __shared__ double d[];            // L
    const DevView &v = c.v;
    const int tid = threadIdx.x, t = blockIdx.x, N = v.N, L = v.L;
    for (int l = tid; l < L; l += 256) d[l] = scale * yf[l + (size_t)L * t];
    __syncthreads();
    const double b = scale * yb[t];
    for (int n = tid; n < N; n += 256) {
        double p = b;
        for (int l0 = 0; l0 < L; l0 += 8) {
            double h[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) h[u] = l0 + u < L ? v.ptdfT[n + (size_t)N * (l0 + u)] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) p += h[u] * (l0 + u < L ? d[l0 + u] : 0.0);
        }
        c.pi[n + (size_t)N * t] = p;
    }
}

// generators. ITER: one PDHG step of every (g,t) of the item; per-item sums of the extrapolated point 2x+ - x.
// !ITER: metrics of the candidate scale * X: per-item sums of x, cost, and sum min(reduced cost, 0) * pmax.
// AV (DOPF_F_GEN_AVAILABILITY contexts): the box's upper end is cap[g,t] = avail_cap(...), the ADMM kernels' product, in the clamp
// and in the reduced-cost term; the row's index is read with mc / pmax, its shape through L2.
template <bool ITER, bool AV = false>
__global__ __launch_bounds__(512) void kc_gen(CentralView c, const double *X, double scale)
{
    __shared__ double red[512];
    const DevView &v = c.v;
    const Item it = v.gen_items[blockIdx.x];
    const int T = v.T, N = v.N, TT = v.genTT, R = v.genR;
    const int tid = threadIdx.x, r = tid / TT, tt = tid - r * TT;
    const double tau = c.tauN[it.node] / c.w;
    double cost = 0.0, dpart = 0.0;
    const double *ftab = nullptr;
    const int *prof = nullptr;
    if constexpr (AV) { ftab = *gen_avail_slot(v); prof = gen_prof(v); }
    for (int tc = 0; tc < T; tc += TT) {
        const int t = tc + tt;
        double acc = 0.0;
        if (r < R && t < T) {
            const double pi = c.pi[it.node + (size_t)N * t];
            for (int g = it.a0 + r; g < it.a1; g += R) {
                const size_t e = (size_t)g * T + t;
                const double mc = v.gen_mc[g];
                double pm = v.gen_pmax[g];
                if constexpr (AV) pm = avail_cap(ftab, T, prof[g], pm, t);
                if (ITER) {
                    const double x0 = v.P[e];
                    const double xn = cs_clamp(x0 - tau * (mc + pi), 0.0, pm);
                    v.P[e] = xn;
                    c.aP[e] += xn;
                    acc += 2.0 * xn - x0;
                } else {
                    const double x = scale * X[e];
                    acc += x;
                    cost += mc * x;
                    dpart += fmin(mc + pi, 0.0) * pm;
                }
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
    if (!ITER) {
        const double csum = block_tree_sum<512>(red, tid, cost, true), dsum = block_tree_sum<512>(red, tid, dpart, false);
        if (tid == 0) { v.part_gcost[blockIdx.x] = csum; c.m_gen[blockIdx.x] = dsum; }
    }
}

// ---- the storage sweeps' slots: what kc_sto and kc_sto_long do for one (storage, timestep), the arithmetic from central_sto.h. The
// kernels keep what differs: who owns t, how the scans' sums arrive, how the item's injections are accumulated. --------------------------
struct StoMetrics {
    double cost = 0.0, dpart = 0.0, viol = 0.0, yterm = 0.0;
};

// the item's cost and c.m_sto[3 item ..]: reduced-cost term, worst level violation, support term
__device__ __forceinline__ void sto_metrics_store(const CentralView &c, const StoMetrics &m, double (*redm)[4], int tid)
{
    double r[4] = {m.cost, m.dpart, m.viol, m.yterm};
    block_metrics<2>(r, redm, tid);
    if (tid == 0) {
        c.v.part_scost[blockIdx.x] = r[0];
        c.m_sto[3 * blockIdx.x + 0] = r[1];
        c.m_sto[3 * blockIdx.x + 1] = r[2];
        c.m_sto[3 * blockIdx.x + 2] = r[3];
    }
}

template <int LV>
__device__ __forceinline__ StoRow sto_row_load(const DevView &v, int s)
{
    const double mc = v.sto_mc[s], pm = v.sto_pmax[s], em = v.sto_emax[s];
    StoRow r{mc, pm, em, 0.0, 0.0, em, 1.0, 1.0};
    if constexpr (LV >= 1) r.e0 = sto_e0(v)[s];                                          // the level before timestep 0
    if constexpr (LV >= 2) { r.elo = sto_end_lo(v)[s]; r.ehi = sto_end_hi(v)[s]; }       // the band of the last one
    if constexpr (LV == 3) { r.al = sto_eff_alpha(v)[s]; r.be = sto_eff_beta(v)[s]; }    // 1 / eta_d, eta_c
    return r;
}

// the columns of timestep t, suf = sum_{tau >= t} yE. ITER: D+, C+ into dn, cn. !ITER: the candidate's cost, reduced-cost and support
// terms into m. Either way dnet is what the slot adds to the level and the injection D - C is returned (ITER: both of the
// extrapolated point).
template <bool ITER, int LV>
__device__ __forceinline__ double sto_primal_slot(const CentralView &c, int node, const StoRow &r, double absH, int t, double suf, double yE,
                                                  double d0, double c0, double &dn, double &cn, double &dnet, StoMetrics &m)
{
    const int T = c.v.T;
    double rD, rC;
    cs_reduced_costs<LV>(r, c.pi[node + (size_t)c.v.N * t], suf, rD, rC);
    if (ITER) {
        cs_column_steps<LV>(r, absH, c.w, T, t, d0, c0, rD, rC, dn, cn);
        const double bd = cs_extra(dn, d0), bc = cs_extra(cn, c0);
        dnet = cs_net<LV>(r, bd, bc);
        return bd - bc;
    }
    dnet = cs_net<LV>(r, d0, c0);
    m.cost += r.mc * (d0 + c0);
    m.dpart += cs_rc_term(rD, rC, r.pm);
    m.yterm = cs_support<LV>(r, yE, t, T, m.yterm);
    return d0 - c0;
}

// the level row of timestep t at element offset e = s T + t; lev: the level before t on entry, after t on return. ITER: the multiplier's
// proximal step, the slot's stores and running sums. !ITER: the candidate's level to v.E, its violation into m.
template <bool ITER, int LV>
__device__ __forceinline__ void sto_level_slot(const CentralView &c, const StoRow &r, size_t e, int t, double yE, double d0, double c0,
                                               double dn, double cn, double &lev, StoMetrics &m)
{
    const DevView &v = c.v;
    const int T = v.T;
    if (ITER) {
        lev += cs_net<LV>(r, cs_extra(dn, d0), cs_extra(cn, c0));
        const double sg = cs_sigma<LV>(r, c.w, t);
        const double yn = cs_prox<LV>(r, yE + sg * lev, sg, t, T);
        v.D[e] = dn; v.C[e] = cn;
        c.yE[e] = yn;
        c.aD[e] += dn; c.aC[e] += cn; c.aE[e] += yn;
    } else {
        lev += cs_net<LV>(r, d0, c0);
        v.E[e] = lev;
        m.viol = fmax(m.viol, cs_violation<LV>(r, lev, t, T));
    }
}

// storages: one wave per storage, lane li owns the K = ceil(T/64) consecutive timesteps li*K .. li*K+K-1 (K <= 8).
// ITER: D+, C+ from the gradient c -+ (pi - sum_{tau >= t} yE), levels of the extrapolated point by a prefix sum, the level
// multipliers' proximal step, running sums. !ITER: metrics of the candidate (scale * XD, XC, XE): cost, reduced-cost term,
// worst level violation, -sum max(yE, 0) e_max; the levels themselves are written to v.E.
// LV (Plan::stoLV; 1: DOPF_F_STO_INITIAL_LEVEL, 2: DOPF_F_STO_TERMINAL_LEVEL, 3: DOPF_F_STO_EFFICIENCY, sto_e0(v) zeros without the first flag): the level
// prefix sums start from e0 (so v.E holds levels that include it), and the row of timestep t lies in [lb_t, ub_t] = [0, e_max],
// with LV 2 [lo, hi] at t = T-1 — that one slot, k = (T-1) % K of lane (T-1) / K. The multiplier's proximal step projects onto
// [lb_t, ub_t] (the row cumsum(C - D) onto [lb_t - e0, ub_t - e0]: the same step, e0 moved to the other side), the violation is
// measured against it, and the dual objective gets the interval's support function sum max(yE, 0) (ub_t - e0) + min(yE, 0) (lb_t - e0):
// with lb_t - e0 != 0 both signs of the multiplier count.
// LV 3 (DOPF_F_STO_EFFICIENCY, dopf_central_solve_lossy): as LV 2 with the level rows e0 + sum_{tau <= t} (be C - al D), be = eta_c =
// sto_eff_beta(v)[s], al = 1 / eta_d = sto_eff_alpha(v)[s] — the one extension that changes K itself. The reduced costs take the
// multipliers' suffix sum with these coefficients (rD = mc + pi - al suf, rC = mc - pi + be suf), D and C get step sizes of their own
// from their columns' sums of |K| (1 + absH + al (T - t), ... + be (T - t)), the row sum of a level row is (al + be) (t + 1), and the
// levels are prefix sums of be C - al D. The injection D - C, the proximal step, the violation and the support-function term are
// those of LV 2 (they are written in the level). Only al and be live across the solve: every use is a multiply. With al = be = 1
// each new operation multiplies by exactly 1 (a fused multiply-add then rounds once, like the addition it stands for): LV 2's bits.
template <bool ITER, int LV = 0>
__global__ __launch_bounds__(256) void kc_sto(CentralView c, const double *XD, const double *XC, const double *XE, double scale)
{
    __shared__ double red[4][64 * KMAX];
    __shared__ double redm[4][4];
    const DevView &v = c.v;
    const Item it = v.sto_items[blockIdx.x];
    const int T = v.T;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = (T + 63) / 64, t0 = lane * K;
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    StoMetrics m;
    const double absH = c.absHn[it.node];
    for (int s = it.a0 + wv; s < it.a1; s += 4) {           // (wave-uniform trip count per wave)
        const StoRow r = sto_row_load<LV>(v, s);
        double yE[KMAX], d0[KMAX], c0[KMAX];
        double ysum = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int t = t0 + k;
            const bool ok = k < K && t < T;
            const size_t e = (size_t)s * T + (ok ? t : 0);
            yE[k] = ok ? (ITER ? c.yE[e] : scale * XE[e]) : 0.0;
            d0[k] = ok ? (ITER ? v.D[e] : scale * XD[e]) : 0.0;
            c0[k] = ok ? (ITER ? v.C[e] : scale * XC[e]) : 0.0;
            ysum += yE[k];
        }
        const double incl = wave_prefix(ysum, lane);
        const double total = __shfl(incl, 63);
        double before = incl - ysum;                          // sum of yE over the steps before this lane's first
        double net = 0.0;
        double dn[KMAX], cn[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int t = t0 + k;
            dn[k] = 0.0; cn[k] = 0.0;
            if (k < K && t < T) {
                const double suf = total - before;            // sum_{tau >= t} yE
                before += yE[k];
                double dnet;
                acc[k] += sto_primal_slot<ITER, LV>(c, it.node, r, absH, t, suf, yE[k], d0[k], c0[k], dn[k], cn[k], dnet, m);
                net += dnet;
            }
        }
        const double inclE = wave_prefix(net, lane);
        double lev = inclE - net;                             // level before this lane's first step
        if constexpr (LV >= 1) lev += r.e0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int t = t0 + k;
            if (k < K && t < T) sto_level_slot<ITER, LV>(c, r, (size_t)s * T + t, t, yE[k], d0[k], c0[k], dn[k], cn[k], lev, m);
        }
    }
    item_sums_store(acc, red, v.part_sinj, K, T, tid, lane, wv);
    if (!ITER) sto_metrics_store(c, m, redm, tid);
}

// ---- the generator row sweeps' slots: what kc_gen_rows and kc_gen_rows_long do for one (generator, timestep) and for a budget row, the
// arithmetic from central_rows.h. The kernels keep what differs: who owns t, how yR[t+1] and xb[t-1] arrive, how the sums are kept. ------
struct GenRow {
    double mc, pm, ru, rd, prev, e_min, e_max, yQ;
    bool ramp, anch, bud;                   // (uniform over the threads that work on the row)
};

struct RowMetrics {
    double cost = 0.0, dpart = 0.0, sup = 0.0, viol = 0.0;
};

// the item's cost and c.m_rows[3 item ..]: reduced-cost term, the rows' support terms, their worst violation
__device__ __forceinline__ void row_metrics_store(const CentralView &c, const RowMetrics &m, double (*redm)[4], int tid)
{
    double r[4] = {m.cost, m.dpart, m.sup, m.viol};
    block_metrics<3>(r, redm, tid);
    if (tid == 0) {
        c.v.part_gcost[blockIdx.x] = r[0];
        c.m_rows[3 * blockIdx.x + 0] = r[1];
        c.m_rows[3 * blockIdx.x + 1] = r[2];
        c.m_rows[3 * blockIdx.x + 2] = r[3];
    }
}

template <bool ITER>
__device__ __forceinline__ GenRow gen_row_load(const CentralView &c, const double *XQ, double scale, int g)
{
    const size_t G = (size_t)c.v.G;
    GenRow r;
    r.mc = c.v.gen_mc[g]; r.pm = c.v.gen_pmax[g];
    r.ru = c.rows_in[g]; r.rd = c.rows_in[G + g]; r.prev = c.rows_in[2 * G + g];
    r.e_min = c.rows_in[3 * G + g]; r.e_max = c.rows_in[4 * G + g];
    r.ramp = cr_has_ramp(r.ru, r.rd, r.prev); r.anch = cr_anchored(r.prev); r.bud = cr_has_budget(r.e_min, r.e_max);
    r.yQ = r.bud ? (ITER ? c.yQ[g] : scale * XQ[g]) : 0.0;
    return r;
}

// the column of timestep t at element offset e = g T + t; y_next: yR[t+1] as the caller found it (read only where t + 1 < T).
// ITER: x+ stored, the extrapolated point returned. !ITER: the candidate's cost and reduced-cost term into m, x returned.
template <bool ITER>
__device__ __forceinline__ double gen_column_slot(const CentralView &c, int node, const GenRow &r, double absH, size_t e, int t, double x0,
                                                  double yR, double y_next, double cap, RowMetrics &m)
{
    const int T = c.v.T;
    if (t + 1 >= T) y_next = 0.0;
    const double rc = cr_reduced_cost(r.mc, c.pi[node + (size_t)c.v.N * t], yR, y_next, r.yQ);
    if (ITER) {
        const double tau = cr_tau(absH, cr_ramp_rows_at(t, T, r.ramp, r.anch), r.bud ? 1 : 0, c.w);
        const double xn = cr_column_step(x0, tau, rc, cap);
        c.v.P[e] = xn;
        c.aP[e] += xn;
        return 2.0 * xn - x0;
    }
    m.cost += r.mc * x0;
    m.dpart += cr_rc_term(rc, cap);
    return x0;
}

// ramp row t (t >= 1, or t = 0 with an anchor) of a generator with ramp rows; xb: the column slot's value at t, x_left: at t - 1
// (t = 0: not read). ITER: the multiplier's proximal step. !ITER: the row's support term and violation into m.
template <bool ITER>
__device__ __forceinline__ void gen_ramp_slot(const CentralView &c, const GenRow &r, size_t e, int t, double yR, double xb, double x_left,
                                              RowMetrics &m)
{
    const double row = t >= 1 ? xb - x_left : xb;
    const double lo = cr_ramp_lo(t, r.rd, r.prev), hi = cr_ramp_hi(t, r.ru, r.prev);
    if (ITER) {
        const double yn = cr_prox(yR, cr_sigma_ramp(t, c.w), row, lo, hi);
        c.yR[e] = yn;
        c.aR[e] += yn;
    } else {
        m.sup += cr_support(yR, lo, hi);
        m.viol = fmax(m.viol, cr_violation(row, lo, hi));
    }
}

// the budget row of generator g, total = sum_t xb[t]; one thread per row calls it
template <bool ITER>
__device__ __forceinline__ void gen_budget_row(const CentralView &c, const GenRow &r, int g, double total, RowMetrics &m)
{
    if (ITER) {
        const double yn = cr_prox(r.yQ, cr_sigma_budget(c.v.T, c.w), total, r.e_min, r.e_max);
        c.yQ[g] = yn;
        c.aQ[g] += yn;
    } else {
        m.sup += cr_support(r.yQ, r.e_min, r.e_max);
        m.viol = fmax(m.viol, cr_violation(total, r.e_min, r.e_max));
    }
}

// generators under ramp and budget rows (dopf_central_solve_coupled; central_rows.h holds the arithmetic, DESIGN.md 5u the rows and
// step sizes): one wave per generator row, four rows of the item in flight per block, lane li owns the K = ceil(T/64) CONSECUTIVE
// timesteps li*K .. li*K+K-1 (K <= 8) as in kc_sto. Consecutive, not lane-interleaved: a ramp row couples t with t - 1, so inside a
// lane both neighbours are registers and only the lane boundary costs a shuffle — one __shfl_up per row for the differences (the
// last slot of lane i-1 feeds the first slot of lane i; that lane is full whenever lane i holds a timestep) and one __shfl_down for
// yR[t+1] in the reduced cost. Interleaved (t = k*64 + lane) every slot would need both. The loads are then strided by K doubles per
// lane, but the K unrolled loads of a wave cover one contiguous range of the row: every cache line fetched is used in full.
// ITER: x+ of every column, the extrapolated point 2x+ - x, the rows' values of it (differences; the row's sum by a wave reduction),
// both multipliers' proximal steps, running sums. !ITER: metrics of the candidate scale * (X, XR, XQ): cost, sum min(rc, 0) cap,
// the rows' support terms and worst violation, per item in c.m_rows. Either way the item's sums over its rows go to part_ginj through
// LDS in a fixed order, as kc_sto's go to part_sinj.
template <bool ITER, bool AV = false>
__global__ __launch_bounds__(256) void kc_gen_rows(CentralView c, const double *X, const double *XR, const double *XQ, double scale)
{
    __shared__ double red[4][64 * KMAX];
    __shared__ double redm[4][4];
    const DevView &v = c.v;
    const Item it = v.gen_items[blockIdx.x];
    const int T = v.T;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = (T + 63) / 64, t0 = lane * K;
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    RowMetrics m;
    const double absH = c.absHn[it.node];
    const double *ftab = nullptr;
    const int *prof = nullptr;
    if constexpr (AV) { ftab = *gen_avail_slot(v); prof = gen_prof(v); }
    for (int g = it.a0 + wv; g < it.a1; g += 4) {           // (wave-uniform trip count per wave)
        const GenRow r = gen_row_load<ITER>(c, XQ, scale, g);
        double x0[KMAX], yR[KMAX], cap[KMAX], xb[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int t = t0 + k;
            const bool ok = k < K && t < T;
            const size_t e = (size_t)g * T + (ok ? t : 0);
            x0[k] = ok ? (ITER ? v.P[e] : scale * X[e]) : 0.0;
            yR[k] = ok && r.ramp ? (ITER ? c.yR[e] : scale * XR[e]) : 0.0;
            cap[k] = r.pm;
            if constexpr (AV) cap[k] = avail_cap(ftab, T, prof[g], r.pm, ok ? t : 0);
        }
        const double y_lane = __shfl_down(yR[0], 1);          // yR of the first step of the next lane (lane 63: never read, t + 1 = T there)
        double lsum = 0.0, last = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int t = t0 + k;
            xb[k] = 0.0;
            if (k < K && t < T) {
                const double y_next = k + 1 < K ? yR[k + 1 < KMAX ? k + 1 : k] : y_lane;
                xb[k] = gen_column_slot<ITER>(c, it.node, r, absH, (size_t)g * T + t, t, x0[k], yR[k], y_next, cap[k], m);
                acc[k] += xb[k];
                lsum += xb[k];
            }
            if (k == K - 1) last = xb[k];
        }
        if (r.ramp) {
            const double x_lane = __shfl_up(last, 1);         // the step before this lane's first (lane 0: t = 0 has no difference)
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int t = t0 + k;
                if (k < K && t < T && (t >= 1 || r.anch))
                    gen_ramp_slot<ITER>(c, r, (size_t)g * T + t, t, yR[k], xb[k], k >= 1 ? xb[k >= 1 ? k - 1 : 0] : x_lane, m);
            }
        }
        if (r.bud) {
            for (int d = 32; d > 0; d >>= 1) lsum += __shfl_xor(lsum, d);      // (a + b = b + a: every lane holds the same bits)
            if (lane == 0) gen_budget_row<ITER>(c, r, g, lsum, m);
        }
    }
    item_sums_store(acc, red, v.part_ginj, K, T, tid, lane, wv);
    if (!ITER) row_metrics_store(c, m, redm, tid);
}

// ---- the long sweeps: rows beyond T = 512 (central_long.h holds the index arithmetic, DESIGN.md 5v the design) ----------------------
// One block of 256 threads works on ONE row at a time and walks it in tiles of 2048 consecutive timesteps; thread i owns the 8
// consecutive steps tile * 2048 + 8 i .. + 7. What kc_sto and kc_gen_rows pass between the lanes of a wave is passed between the
// threads of the block (wave_prefix plus the four waves' totals through LDS, added in a fixed order), and what crosses a tile boundary
// is a block-uniform carry. Element offsets are size_t, so the horizon is bounded by memory alone.

// inclusive prefix sum over the block's 256 threads; total: the block's sum, the same bits in every thread. Every thread calls it.
__device__ __forceinline__ double block_prefix(double x, int lane, int wv, double *wt, double &total)
{
    const double incl = wave_prefix(x, lane);
    __syncthreads();                                          // (the readers of wt in the call before)
    if (lane == 63) wt[wv] = incl;
    __syncthreads();
    const double w0 = wt[0], w1 = wt[1], w2 = wt[2], w3 = wt[3];
    total = ((w0 + w1) + w2) + w3;
    return incl + (wv == 0 ? 0.0 : wv == 1 ? w0 : wv == 2 ? w0 + w1 : (w0 + w1) + w2);
}

// storages on any horizon, in kc_sto's place when the context's plan has stoLong (T > 512, or DOPF_F_DEBUG_LONG_STO): the same LP rows,
// step sizes and metrics — kc_sto's slot functions — ITER, !ITER and LV with kc_sto's meaning. The reduced costs need sum_{tau >= t} yE: one read-only pass over
// the row's yE gives the total, then ONE forward pass over the tiles takes suffix = total - prefix with the sum over the earlier tiles
// as a carry, and in the same tile D+, C+, the extrapolated net, the level prefix (carry: the level at the end of the tile before, e0
// in front of the first) and the multiplier's proximal step. part_sinj[item][t]: the thread that owns t stores for the item's first
// storage and adds for later ones (under Plan::stoLong an item holds one storage).
template <bool ITER, int LV = 0>
__global__ __launch_bounds__(256) void kc_sto_long(CentralView c, const double *XD, const double *XC, const double *XE, double scale)
{
    constexpr int NS = kClSlots;
    __shared__ double wt[4];
    __shared__ double redm[4][4];
    const DevView &v = c.v;
    const Item it = v.sto_items[blockIdx.x];
    const int T = v.T;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tiles = cl_tiles(T);
    StoMetrics m;
    const double absH = c.absHn[it.node];
    double *part = v.part_sinj + (size_t)blockIdx.x * T;
    for (int s = it.a0; s < it.a1; ++s) {                    // (block-uniform)
        const bool first = s == it.a0;
        const StoRow r = sto_row_load<LV>(v, s);
        const size_t row = (size_t)s * T;
        // the row's sum of yE: every thread its own slots, tile after tile, then the block's sum
        double mine = 0.0;
        for (int tile = 0; tile < tiles; ++tile) {
            const long long f = cl_first(tile, tid);
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if (cl_live(f, k, T)) mine += ITER ? c.yE[row + (size_t)(f + k)] : scale * XE[row + (size_t)(f + k)];
        }
        double total;
        block_prefix(mine, lane, wv, wt, total);
        double ycarry = 0.0, lcarry = r.e0;                   // sum of yE over the tiles before; the level at their end
        for (int tile = 0; tile < tiles; ++tile) {
            const long long f = cl_first(tile, tid);
            double yE[NS], d0[NS], c0[NS], dn[NS], cn[NS];
            double ysum = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const bool ok = cl_live(f, k, T);
                const size_t e = row + (ok ? (size_t)(f + k) : 0);
                yE[k] = ok ? (ITER ? c.yE[e] : scale * XE[e]) : 0.0;
                d0[k] = ok ? (ITER ? v.D[e] : scale * XD[e]) : 0.0;
                c0[k] = ok ? (ITER ? v.C[e] : scale * XC[e]) : 0.0;
                ysum += yE[k];
            }
            double tsum;
            const double incl = block_prefix(ysum, lane, wv, wt, tsum);
            double before = ycarry + (incl - ysum);           // sum of yE over the steps before this thread's first
            ycarry += tsum;
            double net = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                dn[k] = 0.0; cn[k] = 0.0;
                if (cl_live(f, k, T)) {
                    const int t = (int)(f + k);
                    const double suf = total - before;        // sum_{tau >= t} yE
                    before += yE[k];
                    double dnet;
                    const double inj = sto_primal_slot<ITER, LV>(c, it.node, r, absH, t, suf, yE[k], d0[k], c0[k], dn[k], cn[k], dnet, m);
                    net += dnet;
                    part[t] = first ? inj : part[t] + inj;
                }
            }
            double ntot;
            const double inclE = block_prefix(net, lane, wv, wt, ntot);
            double lev = lcarry + (inclE - net);              // level before this thread's first step
            lcarry += ntot;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                if (cl_live(f, k, T)) {
                    const int t = (int)(f + k);
                    sto_level_slot<ITER, LV>(c, r, row + (size_t)t, t, yE[k], d0[k], c0[k], dn[k], cn[k], lev, m);
                }
            }
        }
    }
    if (!ITER) sto_metrics_store(c, m, redm, tid);
}

// generators under ramp and budget rows on any horizon, in kc_gen_rows' place when T > 512 (or DOPF_F_DEBUG_LONG_STO): the item's rows
// one after another, the whole block on one row, every slot through kc_gen_rows' slot functions. A ramp row couples t with t - 1 and
// the column of t reads yR[t+1]:
//   yR[t+1] of a thread's last slot is the next thread's first slot — or, for the tile's last thread, the next tile's — and is read
//   from memory with the thread's own loads, BEFORE the tile's barrier; its owner writes it after that barrier (the next tile's first
//   slot: after the next tile's), so what is read is this iteration's old value;
//   the difference at a thread's first slot takes the left neighbour's last xb through LDS (two buffers in turn: one barrier per tile),
//   at a tile's first slot the tile before's last xb as a carry; t = 0 is today's: no difference without an anchor.
// The budget row's sum is kept per thread across the tiles and summed over the block once per row, after the last tile; its proximal
// step follows there. part_ginj[item][t]: the owning thread stores for the item's first generator and adds for later ones.
template <bool ITER, bool AV = false>
__global__ __launch_bounds__(256) void kc_gen_rows_long(CentralView c, const double *X, const double *XR, const double *XQ, double scale)
{
    constexpr int NS = kClSlots;
    __shared__ double hand[2][kClThreads];
    __shared__ double wsum[4];
    __shared__ double redm[4][4];
    const DevView &v = c.v;
    const Item it = v.gen_items[blockIdx.x];
    const int T = v.T;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tiles = cl_tiles(T);
    RowMetrics m;
    const double absH = c.absHn[it.node];
    const double *ftab = nullptr;
    const int *prof = nullptr;
    if constexpr (AV) { ftab = *gen_avail_slot(v); prof = gen_prof(v); }
    double *part = v.part_ginj + (size_t)blockIdx.x * T;
    int buf = 0;                                              // which half of hand[] this tile writes (block-uniform)
    for (int g = it.a0; g < it.a1; ++g) {                    // (block-uniform)
        const bool first = g == it.a0;
        const GenRow r = gen_row_load<ITER>(c, XQ, scale, g);
        const size_t row = (size_t)g * T;
        double lsum = 0.0, xcarry = 0.0;                      // this thread's share of sum_t xb; the last xb of the tile before
        for (int tile = 0; tile < tiles; ++tile) {
            const long long f = cl_first(tile, tid);
            double x0[NS], yR[NS], cap[NS], xb[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const bool ok = cl_live(f, k, T);
                const size_t e = row + (ok ? (size_t)(f + k) : 0);
                x0[k] = ok ? (ITER ? v.P[e] : scale * X[e]) : 0.0;
                yR[k] = ok && r.ramp ? (ITER ? c.yR[e] : scale * XR[e]) : 0.0;
                cap[k] = r.pm;
                if constexpr (AV) cap[k] = avail_cap(ftab, T, prof[g], r.pm, ok ? (int)(f + k) : 0);
            }
            double y_hand = 0.0;                              // yR of the step behind this thread's last slot
            if (r.ramp && cl_live(f, NS, T)) y_hand = ITER ? c.yR[row + (size_t)(f + NS)] : scale * XR[row + (size_t)(f + NS)];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                xb[k] = 0.0;
                if (cl_live(f, k, T)) {
                    const int t = (int)(f + k);
                    const double y_next = k + 1 < NS ? yR[k + 1 < NS ? k + 1 : k] : y_hand;
                    xb[k] = gen_column_slot<ITER>(c, it.node, r, absH, row + (size_t)t, t, x0[k], yR[k], y_next, cap[k], m);
                    part[t] = first ? xb[k] : part[t] + xb[k];
                    lsum += xb[k];
                }
            }
            hand[buf][tid] = xb[NS - 1];
            __syncthreads();
            const double x_left = tid ? hand[buf][tid - 1] : xcarry;      // the step before this thread's first (t = 0: never read)
            xcarry = hand[buf][kClThreads - 1];               // (a full tile's last step; behind the last tile nobody reads it)
            buf ^= 1;
            if (r.ramp) {
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    if (cl_live(f, k, T) && (f + k >= 1 || r.anch)) {
                        const int t = (int)(f + k);
                        gen_ramp_slot<ITER>(c, r, row + (size_t)t, t, yR[k], xb[k], k >= 1 ? xb[k >= 1 ? k - 1 : 0] : x_left, m);
                    }
                }
            }
        }
        if (r.bud) {
            for (int d = 32; d > 0; d >>= 1) lsum += __shfl_xor(lsum, d);      // (a + b = b + a: every lane holds the same bits)
            if (lane == 0) wsum[wv] = lsum;
            __syncthreads();
            // (wsum is written again only behind the next row's first barrier)
            if (tid == 0) gen_budget_row<ITER>(c, r, g, (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]), m);
        }
    }
    if (!ITER) row_metrics_store(c, m, redm, tid);
}

// balance and flow rows of one timestep from the nodal sums in v.cons. ITER: the multipliers' steps (balance: free;
// flows: proximal step of the interval's support function) and running sums. !ITER: worst violations and the dual
// objective's terms -yb d_tot - sum |yf| f_max of the candidate scale * (yb, yf).
// RT (dopf_central_solve_coupled with a rating table, on a DOPF_F_LINE_RATING context): the limit of (l,t) is the table's
// v.fmax[l + L*t] — one load, in the proximal step, the violation and the |yf| F term; !RT: dopf_create's limits, as before.
template <bool ITER, bool RT = false>
__global__ __launch_bounds__(256) void kc_dual(CentralView c, const double *yb, const double *yf, double scale)
{
    extern __shared__ double q[];            // N injections | N demands
    __shared__ double red[256];
    const DevView &v = c.v;
    const int tid = threadIdx.x, t = blockIdx.x, N = v.N, L = v.L;
    double *qd = q + N;
    double part = 0.0, dsum = 0.0;
    for (int n = tid; n < N; n += 256) {
        const double dm = v.demand[n + (size_t)N * t];
        const double x = v.cons[n + (size_t)N * t] - dm;
        q[n] = x;
        qd[n] = dm;
        if (!ITER) v.inj[n + (size_t)N * t] = x;
        part += x;
        dsum += dm;
    }
    const double bal = block_tree_sum<256>(red, tid, part, true), dtot = block_tree_sum<256>(red, tid, dsum, true);
    double fviol = 0.0, fterm = 0.0;
    for (int l = tid; l < L; l += 256) {
        double f = 0.0, fd = 0.0;                // flow of the injections, flow of the demand alone
        for (int n0 = 0; n0 < N; n0 += 8) {
            double h[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) h[u] = n0 + u < N ? v.ptdf[l + (size_t)L * (n0 + u)] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                f += h[u] * (n0 + u < N ? q[n0 + u] : 0.0);
                if (!ITER) fd += h[u] * (n0 + u < N ? qd[n0 + u] : 0.0);
            }
        }
        const size_t i = l + (size_t)L * t;
        double F;
        if constexpr (RT) F = v.fmax[i];        // (the rating table of a DOPF_F_LINE_RATING context: [l + L*t])
        else F = line_fmax0(v)[l];              // (dopf_create's limits)
        if (ITER) {
            const double sg = c.w * c.sigF[l];
            const double z = c.yf[i] + sg * f;
            const double yn = z - sg * cs_clamp(z / sg, -F, F);
            c.yf[i] = yn;
            c.af[i] += yn;
        } else {
            v.flow[i] = f;
            fviol = fmax(fviol, fabs(f) - F);
            fterm += fabs(scale * yf[i]) * F + scale * yf[i] * fd;      // the flow rows act on injection = units - demand
        }
    }
    if (ITER) {
        if (tid == 0) {
            const double yn = c.yb[t] + c.w * c.sigB * bal;
            c.yb[t] = yn;
            c.ab[t] += yn;
        }
    } else {
        const double ft = block_tree_sum<256>(red, tid, fterm, true), fv = block_tree_max<256>(red, tid, fviol, false);
        if (tid == 0) {
            c.m_dual[3 * t + 0] = fabs(bal);
            c.m_dual[3 * t + 1] = fv;
            c.m_dual[3 * t + 2] = -scale * yb[t] * dtot - ft;
        }
    }
}

// dst = scale * src (restart to the running average)
__global__ __launch_bounds__(256) void kc_scale_copy(double *dst, const double *src, double scale, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = scale * src[i];
}

// part[block] = sum over the block's share of (a - b)^2, grid-stride, summed in a fixed order (the primal weight's update at a restart
// of dopf_central_solve_coupled: how far the primal and the dual point have moved since the last restart)
__global__ __launch_bounds__(256) void kc_diff_sq(const double *a, const double *b, size_t n, double *part)
{
    __shared__ double red[256];
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double d = a[i] - b[i];
        s += d * d;
    }
    const double sum = block_tree_sum<256>(red, threadIdx.x, s, false);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// the primal rows of the restart: dst = min(scale * src, upper end of the box). The running sum of n iterates inside [0, ub], times
// 1 / n, can round to one ulp above ub; the restart point, and with it the returned point, has to lie in the box like every iterate
// (inside the box the min is the identity: the bits of kc_scale_copy). GEN: rows of P, ub = gen_pmax[g], AV: cap[g,t] as kc_gen<., true>;
// !GEN: rows of D or C, ub = sto_pmax[s].
template <bool GEN, bool AV = false>
__global__ __launch_bounds__(256) void kc_scale_copy_box(CentralView c, double *dst, const double *src, double scale, size_t n)
{
    const DevView &v = c.v;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int T = v.T, a = (int)(i / (size_t)T), t = (int)(i - (size_t)a * T);
    double ub;
    if constexpr (GEN) {
        ub = v.gen_pmax[a];
        if constexpr (AV) ub = avail_cap(*gen_avail_slot(v), T, gen_prof(v)[a], ub, t);
    } else ub = v.sto_pmax[a];
    dst[i] = fmin(scale * src[i], ub);
}

void central_launch_price(const CentralView &c, const double *yb, const double *yf, double scale, hipStream_t s)
{
    hipLaunchKernelGGL(kc_price, dim3(c.v.T), dim3(256), (size_t)c.v.L * sizeof(double), s, c, yb, yf, scale);
}

// the generator / storage sweep of a context: the plan's feature instantiation (genAvail, stoLV), today's without the flags
// (c.rows_in: the ramp and budget rows' sweep in kc_gen's place; XR, XQ: the candidate's multipliers of those rows)
template <bool ITER>
static void launch_gen(const CentralView &c, const Plan &p, const double *X, const double *XR, const double *XQ, double scale, hipStream_t s)
{
    if (!c.v.nGenItems) return;
    if (c.rows_in && c.longRows)            // (T > 512, or DOPF_F_DEBUG_LONG_STO: the whole block on one row, tile after tile)
        with_bool(p.genAvail, [&](auto av) { hipLaunchKernelGGL((kc_gen_rows_long<ITER, decltype(av)::value>), dim3(c.v.nGenItems), dim3(256), 0, s, c, X, XR, XQ, scale); });
    else if (c.rows_in)
        with_bool(p.genAvail, [&](auto av) { hipLaunchKernelGGL((kc_gen_rows<ITER, decltype(av)::value>), dim3(c.v.nGenItems), dim3(256), 0, s, c, X, XR, XQ, scale); });
    else
        with_bool(p.genAvail, [&](auto av) { hipLaunchKernelGGL((kc_gen<ITER, decltype(av)::value>), dim3(c.v.nGenItems), dim3(512), 0, s, c, X, scale); });
}

template <bool ITER>
static void launch_cdual(const CentralView &c, const double *yb, const double *yf, double scale, hipStream_t s)
{
    const size_t lds = 2 * (size_t)c.v.N * sizeof(double);
    with_bool(c.rated != 0, [&](auto rt) { hipLaunchKernelGGL((kc_dual<ITER, decltype(rt)::value>), dim3(c.v.T), dim3(256), lds, s, c, yb, yf, scale); });
}

template <bool ITER>
static void launch_sto(const CentralView &c, const Plan &p, const double *XD, const double *XC, const double *XE, double scale, hipStream_t s)
{
    if (!c.v.nStoItems) return;
    if (p.stoLong)                          // (T > 512, or DOPF_F_DEBUG_LONG_STO: one block per storage, tile after tile)
        with_lv(p.stoLV, [&](auto lv) { hipLaunchKernelGGL((kc_sto_long<ITER, decltype(lv)::value>), dim3(c.v.nStoItems), dim3(256), 0, s, c, XD, XC, XE, scale); });
    else with_lv(p.stoLV, [&](auto lv) { hipLaunchKernelGGL((kc_sto<ITER,decltype(lv)::value>), dim3(c.v.nStoItems), dim3(256), 0, s, c, XD, XC, XE, scale); });
}

void central_launch_iteration(const CentralView &c, const Plan &p, const DevView &vreduce, hipStream_t s)
{
    central_launch_price(c, c.yb, c.yf, 1.0, s);
    launch_gen<true>(c, p, nullptr, nullptr, nullptr, 1.0, s);
    launch_sto<true>(c, p, nullptr, nullptr, nullptr, 1.0, s);
    launch_reduce(vreduce, Plan{}, s);            // (nodal sums and cost: k_reduce, whatever chain the context runs)
    launch_cdual<true>(c, nullptr, nullptr, 1.0, s);
}

void central_launch_metrics(const CentralView &c, const Plan &p, const DevView &vreduce, const double *XP, const double *XD, const double *XC, const double *XE,
                            const double *yb, const double *yf, const double *XR, const double *XQ, double scale, hipStream_t s)
{
    central_launch_price(c, yb, yf, scale, s);
    launch_gen<false>(c, p, XP, XR, XQ, scale, s);
    launch_sto<false>(c, p, XD, XC, XE, scale, s);
    launch_reduce(vreduce, Plan{}, s);            // (nodal sums and cost: k_reduce, whatever chain the context runs)
    launch_cdual<false>(c, yb, yf, scale, s);
}

// part[0 .. central_diff_blocks(n)) = the blocks' sums of (a - b)^2
int central_diff_blocks(size_t n) { return (int)std::min<size_t>(kCentralDiffBlocks, (n + 255) / 256); }
void central_launch_diff_sq(const double *a, const double *b, size_t n, double *part, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(kc_diff_sq, dim3(central_diff_blocks(n)), dim3(256), 0, s, a, b, n, part);
}

void central_launch_scale_copy(double *dst, const double *src, double scale, size_t n, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(kc_scale_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, scale, n);
}

// v.P / v.D / v.C = scale * (aP / aD / aC), kept inside their boxes
void central_launch_scale_copy_primal(const CentralView &c, const Plan &p, double scale, hipStream_t s)
{
    const DevView &v = c.v;
    const size_t GT = (size_t)v.G * v.T, ST = (size_t)v.S * v.T;
    const dim3 gg((unsigned)((GT + 255) / 256)), gs((unsigned)((ST + 255) / 256));
    if (GT) with_bool(p.genAvail, [&](auto av) { hipLaunchKernelGGL((kc_scale_copy_box<true, decltype(av)::value>), gg, dim3(256), 0, s, c, v.P, (const double *)c.aP, scale, GT); });
    if (ST) {
        hipLaunchKernelGGL((kc_scale_copy_box<false>), gs, dim3(256), 0, s, c, v.D, (const double *)c.aD, scale, ST);
        hipLaunchKernelGGL((kc_scale_copy_box<false>), gs, dim3(256), 0, s, c, v.C, (const double *)c.aC, scale, ST);
    }
}

}  // namespace dopf
