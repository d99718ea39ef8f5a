// gen_budget_win.h — dopf_set_generator_energy_budget_windows: the generators' x-update under one energy budget per
// sub-window of the horizon,
//     e_min[g,j] <= sum_{win_end[j-1] <= t < win_end[j]} P[g,t] <= e_max[g,j],
// the launch a DOPF_F2_GEN_ENERGY_BUDGET context runs while a table is set (Plan::genBudgetWin). Included by kernels_agents.hip behind
// gen_budget.h, whose rows (BudgetRowPlate, BudgetRowNet), sums and search (budget_root.h) it runs as they are.
//
// The windows are disjoint, so a row separates into n_win problems with one multiplier each. k_gen_budget's grid, block and phases,
// with a wave per (row, window) unit (budget_win_map.h) where that kernel has a wave per row:
//  1. lanes over the window's timesteps, lane 0 at its first. A free unit stores the clamped step of k_gen_update<LINES, AV, QC>; a
//     budgeted one forms that step's sum over its window, runs budget_root on the window alone and stores x(nu*) there; lane 0 stores
//     the unit's nu (always: dopf_get_generator_budget_window_price). A searched window of one step (of a table with several windows)
//     stores the closed form clamp(clamped step, e_min, min(e_max, cap)) instead of x(nu*): the bound's own bits. A unit reads and
//     writes nothing of its row outside its window, so the units of a row may run in different waves at once. A unit whose search
//     reaches kBudgetMaxEvals keeps its clamped step in that window and counts in Status::solver_fail;
//  2. a barrier;
//  3. the item's sums from the stored rows: k_gen_budget's code, tiling and order.
// With n_win = 1 a unit is a row over [0, T): every address, lane assignment and order of additions is k_gen_budget's, and so are
// the stored bits.
#pragma once

#include "budget_win_map.h"

namespace dopf {

// MN: as k_gen_budget's — the rows' floors behind mnv, the box [fmin(p_min, cap), cap] (dopf_set_generator_budget_min_output),
// in free windows too. The one-step closed form keeps its shape: the clamped step is at or above the floor already, and the setter
// has made sure that e_max >= floor. The MN = false instantiations never read mnv and are the code of before
template <bool LINES, bool AV, bool QC, bool MN>
__global__ __launch_bounds__(512) void k_gen_budget_win(DevView v, BudgetWinView bw, const double *mnv)
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
    const int nw = bw.n_win;

    // (the unit is the wave's: scalar indices, no address registers per lane)
    const int units = (it.a1 - it.a0) * nw;
    for (int u = __builtin_amdgcn_readfirstlane(wave); u < units; u += kBudgetWaves) {
        const BudgetUnit un = budget_win_unit(u, it.a0, nw, bw.end);
        const int g = un.g, t0 = un.t0, t1 = un.t1;
        const size_t at = (size_t)g * nw + un.j;
        const double mc = v.gen_mc[g], pm = v.gen_pmax[g];
        const double elo = bw.emin[at], ehi = bw.emax[at];
        const int pr = AV ? prof[g] : -1;
        double c2 = 0.0, iq = inv;
        if constexpr (QC) { c2 = c2v[g]; iq = 1.0 / ((w + gam) + c2); }
        double pmn = 0.0;
        if constexpr (MN) pmn = mnv[g];
        double *Prow = v.P + (size_t)g * T;
        const BudgetRowPlate<AV, QC, MN> plate{v.price, v.s, Prow, ftab, gam, inv, c2, iq, pm, it.node, N, T, pr, pmn};
        const BudgetRowNet<AV, QC, MN> net{&v, Prow, ftab, w, c2, pm, it.node, N, T, pr, pmn};
        auto step = [&](int t, double mce, double &p0, int &piece) {
            if constexpr (LINES) return net.step(t, mce, p0, piece);
            else return plate.step(t, mce, p0, piece);
        };
        double nu = 0.0;
        if (!(elo <= 0.0 && ehi == INFINITY)) {
            // the clamped step's sum over the window
            double part = 0.0, p0;
            int piece;
            for (int t = t0 + lane; t < t1; t += 64) part += step(t, mc, p0, piece);
            const double phi0 = budget_wave_sum(part);
            // the search, by the whole wave (a lane without a timestep of the window adds 0.0 and agrees with every test)
            auto probe = [&](double a, double m, double b) {
                double sum = 0.0;
                BudgetSame sm;
                for (int t = t0 + lane; t < t1; t += 64) {
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
            // |nu*| >= |phi(0) - bound| / (the window's length x the largest slope of a timestep); never below a price's resolution
            const double off = phi0 > ehi ? phi0 - ehi : elo - phi0;
            const double first = fmax(off / ((double)(t1 - t0) * (LINES ? net.slope() : plate.slope())), 1e-12);
            int evals = 0;
            const int rc = budget_root(probe, phi0, elo, ehi, first, kBudgetMaxEvals, &nu, &evals);
            if (rc < 0) {
                nu = 0.0;                                    // the clamped step stays in the window
                if (lane == 0) atomicAdd(&v.st->solver_fail, 1ull);
            }
        }
        // the window, stored once: the clamped step (nu == 0: gen_mc itself, the bits of k_gen_update) or x(nu*). A searched window of
        // one step among several has its minimiser in closed form — the clamped step moved into [e_min, min(e_max, cap)] — and stores
        // that: the bound itself, not x(nu*), which meets it only up to the rounding of gen_mc + nu (nu stays the search's). One
        // window over a one-step horizon stays on k_gen_budget's path, bit for bit
        const double mce = nu == 0.0 ? mc : mc + nu;
        const bool one = nw > 1 && t1 - t0 == 1 && nu != 0.0;
        for (int t = t0 + lane; t < t1; t += 64) {
            double p0;
            int piece;
            double pn = step(t, mce, p0, piece);
            if (one) pn = fmin(fmax(step(t, mc, p0, piece), elo), fmin(ehi, LINES ? net.cap(t) : plate.cap(t)));
            Prow[t] = pn;
            if constexpr (LINES) {
                if (v.keepDeltas || v.walk_any[t]) v.dltG[(size_t)g * T + t] = pn - p0;
            }
        }
        // the window's price, behind the store loop as in k_gen_budget<.., PR = true>
        if (lane == 0) bw.nu[at] = nu;
    }
    __syncthreads();

    // the item's sums, from the rows as stored: k_gen_budget's (k_gen_update's) tiling and order of additions
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

void launch_gen_budget_win(const DevView &v, const Plan &p, hipStream_t s)
{
    if (v.nGenItems == 0) return;
    with_bool(v.L > 0, [&](auto ln) {
        with_bool(p.genAvail, [&](auto av) {
            with_bool(p.genQuad, [&](auto qc) {
                with_bool(p.genBudgetMinOut != nullptr, [&](auto mn) {
                    hipLaunchKernelGGL((k_gen_budget_win<decltype(ln)::value, decltype(av)::value, decltype(qc)::value, decltype(mn)::value>),
                                       dim3(v.nGenItems), dim3(512), 0, s, v, p.genBudgetWin, (const double *)p.genBudgetMinOut);
                });
            });
        });
    });
}

}  // namespace dopf
