// gen_ramp_budget.h — DOPF_F2_GEN_RAMP_BUDGET (copper plates): the generators' x-update under ramp limits and energy
// budgets at once, a launch of its own. Included by kernels_agents.hip behind gen_ramp.h and gen_budget.h, whose pieces it runs
// (ramp_repair, BudgetRowPlate, budget_root); the pair's own search is ramp_budget.h.
//
// One block per generator item, kRampWaves waves, a wave per row. A row falls through a cascade:
//  1. lanes over t: the clamped step of k_gen_update<false, AV, QC>, its centres c_t (LDS up to T = kRampLdsT, the wave's scratch
//     beyond), its sum (k_gen_budget's order) and every difference of neighbours against the ramps. A step that keeps ramps and
//     budget is stored: the bits of k_gen_update;
//  2. it keeps the ramps but not the budget: budget_root, exactly as k_gen_budget runs it. x(nu*) of the relaxed problem is the
//     pair's minimiser where it keeps the ramps, and is stored: the bits of k_gen_budget;
//  3. it breaks a ramp: ramp_repair on lane 0, as k_gen_ramp runs it. Where its sum keeps the budget the row is done: the bits of
//     k_gen_ramp;
//  4. otherwise the pair search: every lane runs the serial programme for a candidate multiplier of its own (ramp_budget_run), its
//     y* and knots interleaved [slot][lane] in the wave's scratch — lanes at the same slot touch one line — sums and signatures
//     travel by shuffles, and the search (ramp_budget_search) is the same on every lane. The row stored is the programme's own output
//     at nu*, written by lane 0. A row whose search gives up keeps its step at nu = 0 and counts in Status::solver_fail.
// Lane 0 stores the multiplier the storing branch put on the budget row behind the scratch (gen_budget_price(v, true)): 0 from 1 and
// 3, nu* from 2 and 4, 0 where a search gave up.
// Then the item's sums from the stored rows, in k_gen_update's order with its tiling: the same bits whenever the rows are.
#pragma once

#include "ramp_budget.h"

namespace dopf {

// a lane's candidate: the programme on the wave's shared centres, with the lane's own work arrays
template <bool AV>
struct RampBudgetBatch {
    const double *c, *ftab;
    double *work;                   // the wave's [slot][lane] scratch: y*[T] | kx[2T + 2] | kv[2T + 2]
    double q, up, down, prev, pm;
    int T, prof, lane;
    double phi_;
    unsigned long long sig_;
    struct Cap {
        const double *ftab;
        double pm;
        int T, prof;
        __device__ __forceinline__ double operator()(int t) const { return AV ? avail_cap(ftab, T, prof, pm, t) : pm; }
    };
    __device__ __forceinline__ bool run(double nu, double *out)
    {
        const int K = 2 * T + 2;
        const RbSpan y{work + lane, 64}, kx{work + (size_t)T * 64 + lane, 64}, kv{work + ((size_t)T + K) * 64 + lane, 64};
        const bool ok = ramp_budget_run(c, nu / q, Cap{ftab, pm, T, prof}, T, q, up, down, prev, y, kx, kv, K, out, &phi_, &sig_);
        if (!ok) phi_ = __builtin_nan("");
        return ok;
    }
    __device__ __forceinline__ void eval(int kind, double a, double b, int n) { run(rb_candidate(kind, a, b, n == 1 ? 0 : lane), nullptr); }
    __device__ __forceinline__ double phi(int j) const { return __shfl(phi_, j); }
    __device__ __forceinline__ unsigned long long sig(int j) const
    {
        const unsigned lo = __shfl((unsigned)sig_, j), hi = __shfl((unsigned)(sig_ >> 32), j);
        return ((unsigned long long)hi << 32) | lo;
    }
};

// RP (dopf_get_generator_ramp_price): the rows' ramp multipliers go into rpv, T doubles per row in sorted order. By
// branch: 1 and 2 (the ramps kept) zeros; 3 where its sum keeps the budget: ramp_price of the repaired row (shift 0); 4: ramp_price of
// the programme's row under its nu (shift = nu / q), zeros where the search gave up. cs keeps the centres, the row's kx / kv are free
// behind the repair and behind bt.run. RP = false (rpv unused) is the code of before
template <bool AV, bool QC, bool RP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(6))) void k_gen_ramp_budget(DevView v, double *rpv)
{
    if (v.st->halt) return;
    constexpr int NK = 2 * kRampLdsT + 2;
    __shared__ double red[512];
    __shared__ double s_c[kRampWaves][kRampLdsT], s_cy[kRampWaves][kRampLdsT], s_kx[kRampWaves][NK], s_kv[kRampWaves][NK];
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
    const double *emin = gen_rb_min(v), *emax = gen_rb_max(v);
    double *const nuv = gen_budget_price(v, true);

    // the wave's scratch: c[T] (read beyond kRampLdsT only) | the 64 lanes' work arrays, whose head serves ramp_repair beyond kRampLdsT
    double *wsc = gen_rb_scratch(v) + ((size_t)blockIdx.x * kRampWaves + wave) * ramp_budget_wave_doubles(T);
    double *work = wsc + T;
    double *cs = s_c[wave], *cy = s_cy[wave], *kx = s_kx[wave], *kv = s_kv[wave];
    if (T > kRampLdsT) {
        cs = wsc;
        cy = work;
        kx = cy + T;
        kv = kx + 2 * (size_t)T + 2;
    }

    for (int g = it.a0 + wave; g < it.a1; g += kRampWaves) {
        const double mc = v.gen_mc[g], pm = v.gen_pmax[g];
        const double up = upv[g], dn = dnv[g], prev = pvv[g];
        const double elo = emin[g], ehi = emax[g];
        const int pr = AV ? prof[g] : -1;
        double c2 = 0.0, iq = inv;
        if constexpr (QC) { c2 = c2v[g]; iq = 1.0 / ((w + gam) + c2); }
        double *Prow = v.P + (size_t)g * T;
        const BudgetRowPlate<AV, QC> plate{v.price, v.s, Prow, ftab, gam, inv, c2, iq, pm, it.node, N, T, pr};
        // one pass over the row, lanes over t: the step at the marginal cost mce (P keeps the proximal centre), its sum in
        // k_gen_budget's order, whether a ramp is broken; KEEP: the centres into cs; STORE: the step into P
        auto sweep = [&](double mce, bool keep, bool store, double &sum) {
            double left = prev, part = 0.0;
            bool bad = false;
            for (int tc = 0; tc < T; tc += 64) {
                const int t = tc + lane;
                double pn = 0.0;
                if (t < T) {
                    double p0;
                    int piece;
                    pn = plate.step(t, mce, p0, piece);
                    part += pn;
                    if (keep) {
                        // (the expressions of plate.step at mc: the centre k_gen_ramp keeps)
                        const double psum = v.price[it.node + N * t] + gam * v.s[t];
                        if constexpr (QC) cs[t] = p0 - fma(mc + c2 * p0, iq, psum * iq);
                        else cs[t] = p0 - fma(mc, inv, psum * inv);
                    }
                    if (store) Prow[t] = pn;
                }
                double before = __shfl_up(pn, 1);
                if (lane == 0) before = left;
                if (t < T && before == before) {
                    const double d = pn - before;
                    bad = bad || d > up || -d > dn;
                }
                left = __shfl(pn, 63);
            }
            sum = budget_wave_sum(part);
            return __any(bad) != 0;
        };
        const bool budgeted = !(elo <= 0.0 && ehi == INFINITY);
        double phi0;
        // (a row with default budgets stores at once, as k_gen_ramp does: nothing reads its proximal centre again)
        const bool bad0 = sweep(mc, true, !budgeted, phi0);
        const bool in0 = !budgeted || (phi0 >= elo && phi0 <= ehi);
        bool pair = false;
        // the row's budget price (dopf_get_generator_budget_price): what the branch that stores the row put on its budget row
        double rowNu = 0.0;
        // RP: the shift of the centres under which the stored row is a ramp projection (NaN: its ramps were kept, or its search gave up)
        double rpShift = __builtin_nan("");
        if (!bad0 && in0) {
            if (budgeted) sweep(mc, false, true, phi0);         // 1. the clamped step
        } else if (!bad0) {
            // 2. the budget alone, as k_gen_budget searches it
            auto probe = [&](double a, double m, double b) {
                double sum = 0.0;
                BudgetSame sm;
                for (int t = lane; t < T; t += 64) {
                    int pa, pmid, pb;
                    double q0;
                    plate.step(t, mc + a, q0, pa);
                    sum += plate.step(t, mc + m, q0, pmid);
                    plate.step(t, mc + b, q0, pb);
                    sm.add(pa, pmid, pb);
                }
                return BudgetProbe{budget_wave_sum(sum), __all(sm.sameA) != 0, __all(sm.sameB) != 0, __all(sm.atLo) != 0,
                                   __all(sm.atHi) != 0};
            };
            const double off = phi0 > ehi ? phi0 - ehi : elo - phi0;
            const double first = fmax(off / ((double)T * plate.slope()), 1e-12);
            double nu = 0.0, sum;
            int evals = 0;
            const int rc = budget_root(probe, phi0, elo, ehi, first, kBudgetMaxEvals, &nu, &evals);
            if (rc < 0) {
                if (lane == 0) atomicAdd(&v.st->solver_fail, 1ull);
                sweep(mc, false, true, sum);                    // the clamped step stays in the row (it keeps the ramps)
            } else if (!sweep(mc + nu, false, false, sum)) {
                sweep(mc + nu, false, true, sum);               // the relaxed problem's minimiser keeps the ramps: optimal
                rowNu = nu;
            } else {
                pair = true;
            }
        } else {
            // 3. the ramps alone, as k_gen_ramp repairs them (cs keeps the centres: ramp_repair overwrites its own copy)
            for (int t = lane; t < T; t += 64) cy[t] = cs[t];
            __threadfence_block();
            if (lane == 0)
                ramp_repair<AV>(Prow, cy, kx, kv, T, (w + gam) + c2, fmin(up, pm), fmin(dn, pm), prev, pm, ftab, pr);
            __threadfence_block();
            if (budgeted) {
                double part = 0.0;
                for (int t = lane; t < T; t += 64) part += Prow[t];
                phi0 = budget_wave_sum(part);
                pair = !(phi0 >= elo && phi0 <= ehi);
            }
            if constexpr (RP) { if (!pair) rpShift = 0.0; }
        }
        if (pair) {
            // 4. the pair search: phi0 is the sum of the step at nu = 0, which breaks the budget
            __threadfence_block();                              // the wave's centres, before every lane reads them
            const double q = (w + gam) + c2;
            RampBudgetBatch<AV> bt{cs, ftab, work, q, fmin(up, pm), fmin(dn, pm), prev, pm, T, pr, lane, 0.0, 0ull};
            const double off = phi0 > ehi ? phi0 - ehi : elo - phi0;
            const double first = fmax(off / ((double)T * plate.slope()), 1e-12);
            const double tol = 1e-12 * (1.0 + (double)T * pm);
            double nu = 0.0;
            int rounds = 0;
            const int rc = ramp_budget_search(bt, phi0, elo, ehi, first, tol, kRampBudgetMaxRounds, &nu, &rounds);
            bool ok = rc == 1;
            if (ok && lane == 0) ok = bt.run(nu, Prow);
            ok = __shfl((int)ok, 0) != 0;
            if (ok) rowNu = nu;
            if constexpr (RP) { if (ok) rpShift = nu / q; }
            if (!ok) {
                if (lane == 0) atomicAdd(&v.st->solver_fail, 1ull);
                double sum;
                if (!bad0) sweep(mc, false, true, sum);          // (from 2: P still holds the proximal centre; from 3: the repaired row)
            }
            __threadfence_block();
        }
        if (lane == 0) nuv[__builtin_amdgcn_readfirstlane(g)] = rowNu;       // (g is the wave's: a scalar index)
        if constexpr (RP) {
            double *rrow = rpv + (size_t)__builtin_amdgcn_readfirstlane(g) * T;
            if (rpShift == rpShift) {
                // (the stored ramps: an infinite one is never tight; no floors on a budget context)
                const RampCap<AV> cap{ftab, pm, T, pr};
                if (lane == 0)
                    ramp_price(Prow, cs, rpShift, (w + gam) + c2, RampFloor<AV, false>{cap, 0.0}, cap, T, up, dn, prev, pm, kx, kv, rrow);
            } else {
                for (int t = lane; t < T; t += 64) rrow[t] = 0.0;
            }
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

void launch_gen_ramp_budget(const DevView &v, const Plan &p, hipStream_t s)
{
    if (v.nGenItems == 0) return;
    with_bool(p.genAvail, [&](auto av) {
        with_bool(p.genQuad, [&](auto qc) {
            with_bool(p.genRampPrice != nullptr, [&](auto rp) {
                hipLaunchKernelGGL((k_gen_ramp_budget<decltype(av)::value, decltype(qc)::value, decltype(rp)::value>), dim3(v.nGenItems),
                                   dim3(512), 0, s, v, p.genRampPrice);
            });
        });
    });
}

}  // namespace dopf
