// gen_ramp_net.h — DOPF_F_GEN_RAMP | DOPF_F_GEN_RAMP_NETWORK (networks): the generators' x-update under ramp limits
// where the row's derivative per step is mc + c2 x + Psi_{n,t}(x - p0) + w (x - p0), piecewise linear with the kinks of the node's table.
// Included by gen_ramp.h (kernels_agents.hip: clampd, rcp64, the helpers of dopf_internal.h); the programme itself is ramp_dp.h.
//
// k_gen_ramp's shape: one block per generator item (all its rows sit at one node and share its tables), kRampWaves waves, three phases:
//  1. a wave per row, lanes over t: the step of gen_lines_body<512, 4, AV, QC>, expression by expression, is stored to P (and to dltG
//     where the slack sums walk the agents), p0 is kept (the row is overwritten in place and the repair needs the old values) and
//     every difference of neighbours is held against the ramps; the wave sums the tables' kink counts m_t;
//  2. a row whose clamped step keeps its ramps is optimal and done. For the others lane 0 runs ramp_repair_pwl — knots in LDS where
//     T <= kRampLdsT and 2T + 2 + sum m_t fit, else in the wave's scratch behind gen_pmax (capacity ramp_net_knots) — and the wave
//     rewrites the row AND its dltG entries. A row whose knots exceed the capacity keeps its clamped step and counts in
//     Status::solver_fail (dopf_iterate: DOPF_E_SOLVER);
//  3. the item's sums from the stored rows, in gen_lines_body's order with its tiling, into part_T and part_gcost: the bits of
//     k_gen_update<true, AV, QC> whenever the rows are.
#pragma once

#include "ramp_dp.h"

namespace dopf {

constexpr int kRampNetLdsKnots = 2 * kRampLdsT + 2 + 62;        // knots per wave in LDS: 320 (61.5 KB per block with p0, y*, red)

// what ramp_repair_pwl asks of a row: its caps and the tables of its node
template <bool AV>
struct RampRowTab {
    const double *tb_beta, *tb_psi, *tb_slope, *tb_psi0;
    const int *tb_m;
    const double *p0, *ftab;
    size_t node, N;
    int M2, T, prof;
    double mc, c2, w, pm;
    double pmn;                     // the row's p_min (read by floor() only: ramp_repair_pwl<true>)
    __device__ __forceinline__ double cap(int t) const { return AV ? avail_cap(ftab, T, prof, pm, t) : pm; }
    __device__ __forceinline__ double floor(int t) const { return fmin(pmn, cap(t)); }
    __device__ __forceinline__ RampStepTab step(int t) const
    {
        const size_t at = node + N * (size_t)t;
        return RampStepTab{tb_m[at], tb_beta + at * M2, tb_psi + at * M2, tb_slope + at * (M2 + 1), tb_psi0[at], p0[t], mc, c2, w};
    }
};

// MN: as k_gen_ramp's — the box is [fmin(p_min, cap), cap] (dopf_set_generator_min_output)
template <bool AV, bool QC, bool MN>
__global__ __launch_bounds__(512) void k_gen_ramp_net(DevView v)
{
    if (v.st->halt) return;
    constexpr int NK = kRampNetLdsKnots;
    __shared__ double red[512];
    __shared__ double s_p0[kRampWaves][kRampLdsT], s_cy[kRampWaves][kRampLdsT], s_kx[kRampWaves][NK], s_kv[kRampWaves][NK];
    const Item it = v.gen_items[blockIdx.x];
    const int T = v.T, N = v.N;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double w = v.w_prox;
    const double *ftab = nullptr;
    const int *prof = nullptr;
    if constexpr (AV) { ftab = *gen_avail_slot(v); prof = gen_prof(v); }
    const double *c2v = nullptr;
    if constexpr (QC) c2v = gen_c2(v);
    const double *upv = gen_ramp_up(v), *dnv = gen_ramp_down(v), *pvv = gen_ramp_prev(v);
    const double *mnv = nullptr;
    if constexpr (MN) mnv = gen_min_output(v);

    // the wave's scratch: p0[T] | y*[T] | kx[K] | kv[K]
    const int K = ramp_net_knots(T, v.L);
    double *const scr = gen_ramp_scratch(v) + ((size_t)blockIdx.x * kRampWaves + wave) * ramp_net_row_doubles(T, v.L);
    double *p0s = s_p0[wave], *cy = s_cy[wave];
    if (T > kRampLdsT) { p0s = scr; cy = scr + T; }

    for (int g = it.a0 + wave; g < it.a1; g += kRampWaves) {
        const double mc = v.gen_mc[g], pm = v.gen_pmax[g];
        const double up = upv[g], dn = dnv[g], prev = pvv[g];
        const int pr = AV ? prof[g] : -1;
        double c2 = 0.0, pmn = 0.0;
        if constexpr (QC) c2 = c2v[g];
        if constexpr (MN) pmn = mnv[g];
        double *Prow = v.P + (size_t)g * T;
        double left = prev;                         // the value in front of the chunk's first timestep (NaN: none)
        bool bad = false;
        int msum = 0;
        for (int tc = 0; tc < T; tc += 64) {
            const int t = tc + lane;
            double pn = 0.0;
            if (t < T) {
                // the step of gen_lines_body: one binary search over the node's table, one linear solve
                const size_t at = (size_t)it.node + (size_t)N * t;
                const int m = v.tb_m[at];
                const double *beta = v.tb_beta + at * v.M2, *psi = v.tb_psi + at * v.M2;
                const double *slope = v.tb_slope + at * (v.M2 + 1);
                const double psi0 = v.tb_psi0[at];
                const double slope0 = slope[0];
                const double inv0 = rcp64(slope0 + w);
                const bool keepd = v.keepDeltas || v.walk_any[t];
                const double p0 = Prow[t];
                const double cap = AV ? avail_cap(ftab, T, pr, pm, t) : pm;
                double dl;
                if constexpr (QC) {
                    const double mq = mc + c2 * p0, wq = w + c2;
                    if (m == 0) {
                        dl = -(mq + psi0) * rcp64(slope0 + wq);
                    } else {
                        int lo = 0, hi = m;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (psi[mid] + wq * beta[mid] >= -mq) hi = mid; else lo = mid + 1;
                        }
                        const int a = lo < m ? lo : m - 1;
                        dl = beta[a] - (mq + psi[a] + wq * beta[a]) * rcp64(slope[lo] + wq);
                    }
                } else if (m == 0) {
                    dl = -(mc + psi0) * inv0;
                } else {
                    int lo = 0, hi = m;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (psi[mid] + w * beta[mid] >= -mc) hi = mid; else lo = mid + 1;
                    }
                    const int a = lo < m ? lo : m - 1;
                    dl = beta[a] - (mc + psi[a] + w * beta[a]) * rcp64(slope[lo] + w);
                }
                if constexpr (MN) pn = clampd(p0 + dl, fmin(pmn, cap), cap);
                else pn = clampd(p0 + dl, 0.0, cap);
                Prow[t] = pn;
                if (keepd) v.dltG[(size_t)g * T + t] = pn - p0;
                p0s[t] = p0;
                msum += m;
            }
            double before = __shfl_up(pn, 1);
            if (lane == 0) before = left;
            if (t < T && before == before) {
                const double d = pn - before;
                bad = bad || d > up || -d > dn;
            }
            left = __shfl(pn, 63);
        }
        if (__any(bad)) {
            for (int d = 32; d > 0; d >>= 1) msum += __shfl_xor(msum, d);
            double *kx = scr + 2 * (size_t)T, *kv = kx + K;
            int cap_k = K;
            if (T <= kRampLdsT && 2 * T + 2 + msum <= NK) { kx = s_kx[wave]; kv = s_kv[wave]; cap_k = NK; }
            __threadfence_block();                  // the wave's p0, before lane 0 reads them
            int ok = 1;
            if (lane == 0) {
                const RampRowTab<AV> row{v.tb_beta, v.tb_psi, v.tb_slope, v.tb_psi0, v.tb_m, p0s, ftab, (size_t)it.node, (size_t)N,
                                         v.M2, T, pr, mc, c2, w, pm, pmn};
                ok = ramp_repair_pwl<MN>(row, Prow, cy, kx, kv, cap_k, T, fmin(up, pm), fmin(dn, pm), prev) ? 1 : 0;
                if (!ok) atomicAdd(&v.st->solver_fail, 1ull);       // the clamped step stays in the row
            }
            __threadfence_block();
            if (__shfl(ok, 0)) {
                // the deltas phase 1 wrote, from the row as repaired: the slack sums of flagged timesteps walk the agents through them
                for (int t = lane; t < T; t += 64)
                    if (v.keepDeltas || v.walk_any[t]) v.dltG[(size_t)g * T + t] = Prow[t] - p0s[t];
            }
        }
    }
    __syncthreads();

    // the item's sums, from the rows as stored: gen_lines_body's tiling and order of additions
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
            v.part_T[(size_t)t * v.rowsT + it.row] = sum;
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

void launch_gen_ramp_net(const DevView &v, const Plan &p, hipStream_t s)
{
    if (v.nGenItems == 0) return;
    with_bool(p.genAvail, [&](auto av) {
        with_bool(p.genQuad, [&](auto qc) {
            with_bool(p.genMinOut, [&](auto mn) {
                hipLaunchKernelGGL((k_gen_ramp_net<decltype(av)::value, decltype(qc)::value, decltype(mn)::value>), dim3(v.nGenItems),
                                   dim3(512), 0, s, v);
            });
        });
    });
}

}  // namespace dopf
