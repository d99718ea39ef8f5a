// gen_budget.h — DOPF_F2_GEN_ENERGY_BUDGET: the generators' x-update under energy budgets
//     e_min[g] <= sum_t P[g,t] <= e_max[g],
// a launch of its own on copper plates (LINES = false) and networks (LINES = true, the wide chain included: it reaches the generators
// through launch_gen_update too). Included by kernels_agents.hip behind its kernels (clampd, rcp64, the helpers of dopf_internal.h);
// the search itself is budget_root.h.
//
// With a multiplier nu on the budget row the row's step is the library's own with gen_mc[g] + nu for gen_mc[g]: the clamped closed
// form of gen_update_body on a copper plate, the table search of gen_lines_body on a network. One block per generator item,
// kBudgetWaves waves, in three phases as k_gen_ramp:
//  1. a wave per row, lanes over t (P is agent-major: a row's T values are consecutive). A row with default budgets stores the
//     clamped step of k_gen_update<LINES, AV, QC>, bit for bit, and is done. A budgeted row first forms the sum of that step — lane
//     by lane in t order, then the wave's butterfly: a fixed order — WITHOUT storing it;
//  2. a budgeted row whose sum keeps its budget stores the same clamped step. For the others the whole wave runs budget_root: each
//     lane evaluates its timesteps at the candidates, the sums and the piece tests are wave reductions, every lane holds the same
//     bracket. The row is overwritten last, by x(nu*) — until then P still holds the proximal centre p0, from which a timestep's
//     step is formed again at every candidate (the loads hit the cache the first pass filled): nothing is kept per timestep, no LDS
//     and no scratch, at any T. A row whose search reaches kBudgetMaxEvals keeps its clamped step and counts in Status::solver_fail
//     (dopf_iterate: DOPF_E_SOLVER);
//     In the PR instantiations lane 0 stores the row's nu behind the budgets (gen_budget_price(v, false)): what
//     dopf_get_generator_budget_price hands out;
//  3. the item's sums from the stored rows, in k_gen_update's order with its tiling: the same bits whenever the rows are.
#pragma once

#include "budget_root.h"

namespace dopf {

constexpr int kBudgetWaves = 8;

// a row's step at one timestep with the marginal cost mce (gen_mc[g] + nu; at nu = 0 gen_mc[g] itself): copper plate.
// MN (dopf_set_generator_budget_min_output): the box of step t is [fmin(pmn, cap_t), cap_t] — a floor that follows the cap
// down; pmn is the row's p_min (not read without MN: every expression is the one of before)
template <bool AV, bool QC, bool MN = false>
struct BudgetRowPlate {
    const double *price, *s, *Prow, *ftab;
    double gam, inv, c2, iq, pm;
    int node, N, T, prof;
    double pmn = 0.0;
    __device__ __forceinline__ double cap(int t) const { return AV ? avail_cap(ftab, T, prof, pm, t) : pm; }
    // the expressions of gen_update_body, LINES = false (as k_gen_ramp forms them); piece: the clip state of the unclamped step.
    // Without QC gen_update_body writes mc * inv + shift, shift = psum * inv, which the compiler contracts into fma(mc, inv, shift):
    // the explicit fma below carries those bits only while that contraction holds (a build with -ffp-contract=off would part them;
    // the default-budget tests compare the bits and would say so)
    __device__ __forceinline__ double step(int t, double mce, double &p0, int &piece) const
    {
        const double psum = price[node + N * t] + gam * s[t];
        p0 = Prow[t];
        double c;
        if constexpr (QC) c = p0 - fma(mce + c2 * p0, iq, psum * iq);
        else c = p0 - fma(mce, inv, psum * inv);
        const double cp = cap(t);
        if constexpr (MN) {
            const double fl = fmin(pmn, cp);
            piece = budget_piece(c, fl, cp, 0);
            return clampd(c, fl, cp);
        } else {
            piece = budget_piece(c, cp, 0);
            return clampd(c, 0.0, cp);
        }
    }
    // the largest slope |dx_t / dnu| of a timestep
    __device__ __forceinline__ double slope() const { return QC ? iq : inv; }
};

// ... on a network: the step of gen_lines_body, one binary search over the node's table and one linear solve; piece: the clip state
// and, inside the box, the table's interval. MN: as BudgetRowPlate's
template <bool AV, bool QC, bool MN = false>
struct BudgetRowNet {
    const DevView *v;
    const double *Prow, *ftab;
    double w, c2, pm;
    int node, N, T, prof;
    double pmn = 0.0;
    __device__ __forceinline__ double cap(int t) const { return AV ? avail_cap(ftab, T, prof, pm, t) : pm; }
    __device__ __forceinline__ double step(int t, double mce, double &p0, int &piece) const
    {
        const size_t at = (size_t)node + (size_t)N * t;
        const int m = v->tb_m[at];
        const double *beta = v->tb_beta + at * v->M2, *psi = v->tb_psi + at * v->M2;
        const double *slope = v->tb_slope + at * (v->M2 + 1);
        const double psi0 = v->tb_psi0[at];
        const double slope0 = slope[0];
        const double inv0 = rcp64(slope0 + w);
        p0 = Prow[t];
        double dl;
        int lo = 0;
        if constexpr (QC) {
            const double mq = mce + c2 * p0, wq = w + c2;
            if (m == 0) {
                dl = -(mq + psi0) * rcp64(slope0 + wq);
            } else {
                int hi = m;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (psi[mid] + wq * beta[mid] >= -mq) hi = mid; else lo = mid + 1;
                }
                const int a = lo < m ? lo : m - 1;
                dl = beta[a] - (mq + psi[a] + wq * beta[a]) * rcp64(slope[lo] + wq);
            }
        } else if (m == 0) {
            dl = -(mce + psi0) * inv0;
        } else {
            int hi = m;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (psi[mid] + w * beta[mid] >= -mce) hi = mid; else lo = mid + 1;
            }
            const int a = lo < m ? lo : m - 1;
            dl = beta[a] - (mce + psi[a] + w * beta[a]) * rcp64(slope[lo] + w);
        }
        const double cp = cap(t);
        if constexpr (MN) {
            const double fl = fmin(pmn, cp);
            piece = budget_piece(p0 + dl, fl, cp, lo);
            return clampd(p0 + dl, fl, cp);
        } else {
            piece = budget_piece(p0 + dl, cp, lo);
            return clampd(p0 + dl, 0.0, cp);
        }
    }
    // (Psi is non-decreasing: every piece's slope is at most 1 / (w + c2))
    __device__ __forceinline__ double slope() const { return 1.0 / (w + c2); }
};

__device__ __forceinline__ double budget_wave_sum(double x)
{
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// PR: lane 0 stores every row's multiplier for dopf_get_generator_budget_price. The store measured 0.75 us per iteration on config2
// with default budgets, so it is an instantiation of its own, which a context runs from its first call of that entry on
// (Plan::genBudgetPrice); the PR = false instantiations are the code of before.
// MN: the rows' floors are read from mnv (Plan::genBudgetMinOut: G doubles of the context's own, sorted order) and the box is
// [fmin(p_min, cap), cap] in the clamped step, the search and the stored row alike — a row with default budgets stores
// clampd(c, floor, cap). p_min is one value per row, the wave's scalar like mc and pm. The MN = false instantiations never read
// mnv (null then) and are the code of before
template <bool LINES, bool AV, bool QC, bool PR, bool MN>
__global__ __launch_bounds__(512) void k_gen_budget(DevView v, const double *mnv)
{
    if (v.st->halt) return;
    __shared__ double red[512];
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
    const double *emin = gen_budget_min(v), *emax = gen_budget_max(v);

    for (int g = it.a0 + wave; g < it.a1; g += kBudgetWaves) {
        const double mc = v.gen_mc[g], pm = v.gen_pmax[g];
        const double elo = emin[g], ehi = emax[g];
        const int pr = AV ? prof[g] : -1;
        double c2 = 0.0, iq = inv;
        if constexpr (QC) { c2 = c2v[g]; iq = 1.0 / ((w + gam) + c2); }
        double pmn = 0.0;
        if constexpr (MN) pmn = mnv[g];
        double *Prow = v.P + (size_t)g * T;
        // (both row types are cheap to fill; the one the kernel does not use folds away)
        const BudgetRowPlate<AV, QC, MN> plate{v.price, v.s, Prow, ftab, gam, inv, c2, iq, pm, it.node, N, T, pr, pmn};
        const BudgetRowNet<AV, QC, MN> net{&v, Prow, ftab, w, c2, pm, it.node, N, T, pr, pmn};
        auto step = [&](int t, double mce, double &p0, int &piece) {
            if constexpr (LINES) return net.step(t, mce, p0, piece);
            else return plate.step(t, mce, p0, piece);
        };
        double nu = 0.0;
        if (!(elo <= 0.0 && ehi == INFINITY)) {
            // phase 1, budgeted row: the clamped step's sum
            double part = 0.0, p0;
            int piece;
            for (int t = lane; t < T; t += 64) part += step(t, mc, p0, piece);
            const double phi0 = budget_wave_sum(part);
            // phase 2: the search, by the whole wave
            auto probe = [&](double a, double m, double b) {
                double sum = 0.0;
                BudgetSame sm;
                for (int t = lane; t < T; t += 64) {
                    int pa, pmid, pb;
                    double q0;
                    step(t, mc + a, q0, pa);
                    sum += step(t, mc + m, q0, pmid);
                    step(t, mc + b, q0, pb);
                    sm.add(pa, pmid, pb);
                }
                return BudgetProbe{budget_wave_sum(sum), __all(sm.sameA) != 0, __all(sm.sameB) != 0, __all(sm.atLo) != 0,
                                   __all(sm.atHi) != 0};
            };
            // |nu*| >= |phi(0) - bound| / (T x the largest slope of a timestep); never below a price's resolution
            const double off = phi0 > ehi ? phi0 - ehi : elo - phi0;
            const double first = fmax(off / ((double)T * (LINES ? net.slope() : plate.slope())), 1e-12);
            int evals = 0;
            const int rc = budget_root(probe, phi0, elo, ehi, first, kBudgetMaxEvals, &nu, &evals);
            if (rc < 0) {
                nu = 0.0;                                    // the clamped step stays in the row
                if (lane == 0) atomicAdd(&v.st->solver_fail, 1ull);
            }
        }
        // the row, stored once: the clamped step (nu == 0: gen_mc itself, the bits of k_gen_update) or x(nu*)
        const double mce = nu == 0.0 ? mc : mc + nu;
        for (int t = lane; t < T; t += 64) {
            double p0;
            int piece;
            const double pn = step(t, mce, p0, piece);
            Prow[t] = pn;
            if constexpr (LINES) {
                if (v.keepDeltas || v.walk_any[t]) v.dltG[(size_t)g * T + t] = pn - p0;
            }
        }
        // PR: the row's budget price (dopf_get_generator_budget_price): 0.0 for a row with default budgets, one whose step at nu = 0
        // keeps its budget and one whose search gave up, else nu*. Behind the row's store loop: in front of it the wait that opens
        // the loop would cover the store's round trip. g is the wave's: a scalar index, no address registers per lane
        if constexpr (PR) {
            if (lane == 0) gen_budget_price(v, false)[__builtin_amdgcn_readfirstlane(g)] = nu;
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
            if constexpr (LINES) v.part_T[(size_t)t * v.rowsT + it.row] = sum;
            else v.part_ginj[(size_t)blockIdx.x * T + t] = sum;
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

void launch_gen_budget(const DevView &v, const Plan &p, hipStream_t s)
{
    if (v.nGenItems == 0) return;
    with_bool(v.L > 0, [&](auto ln) {
        with_bool(p.genAvail, [&](auto av) {
            with_bool(p.genQuad, [&](auto qc) {
                with_bool(p.genBudgetPrice, [&](auto pr) {
                    with_bool(p.genBudgetMinOut != nullptr, [&](auto mn) {
                        hipLaunchKernelGGL((k_gen_budget<decltype(ln)::value, decltype(av)::value, decltype(qc)::value, decltype(pr)::value,
                                                         decltype(mn)::value>),
                                           dim3(v.nGenItems), dim3(512), 0, s, v, (const double *)p.genBudgetMinOut);
                    });
                });
            });
        });
    });
}

}  // namespace dopf
