// sto_long.h — storages on horizons beyond one lane group (DOPF_F_LONG_HORIZON; included by kernels_agents.hip).
//
// The scan body (sto_cold_body) gives a storage one group of at most 64 lanes x 8 consecutive timesteps: one wave, T <= 512.
// This body runs the SAME price-threshold recursion — backwards over constant-price segments; per segment one scan of the
// clamp-add maps e -> clamp(e + x_t(nu), 0, emax) finds the last open timestep whose unclamped level leaves [0, emax], then a
// bracketed Newton / bisection puts that level on its bound (same tolerances, bracket rules and iteration cap) — with a whole
// block per storage and the horizon cut into TILES of 256 threads x kLongNCH consecutive timesteps:
//   - a scan walks the tiles of [0, lim] in order; inside a tile the lanes compose their steps' maps, the waves scan the lane
//     composites with DPP (scan_maps<64>), one LDS round composes the four wave composites behind the level the tile starts at
//     (the composed map of every tile before it), and the tile's exit level is carried to the next one;
//   - what the recursion needs of a scan — the unclamped level at ONE timestep (the root search's, or the last one out of the
//     band), its slope in nu (sum of dx_t/dnu over the run of unclamped steps that ends there) and the nearest kink in either
//     direction over that run (the way out of a flat piece) — is formed on the fly: per wave in registers, per tile in a second
//     LDS round, across tiles by a carry ("since the last clamped step") — no per-timestep scratch;
//   - the inputs (D0, C0, prices or the Psi tables) are re-read from global memory on every scan, and the prices the recursion
//     assigns go to nu_prev in place: no limit on T but device memory.
// After a root search converges the next scan classifies at the same price (the scan body reuses the one it has in registers):
// one scan more per contact, the same decisions. Two runs give the same bits: every sum is formed in a fixed order.
#pragma once

namespace dopf {

constexpr int kLongNCH = 8;                         // consecutive timesteps per lane (registers: 5 arrays of them)
constexpr int kLongBS = 256;                        // 4 waves
constexpr int kLongWaves = kLongBS / 64;
constexpr int kLongWaveSteps = 64 * kLongNCH;       // 512
constexpr int kLongTile = kLongBS * kLongNCH;       // 2048 timesteps per tile

// what one scan reports about its candidate timestep (block-uniform)
struct LongCand {
    int o;              // the timestep (-1: none)
    double sv;          // its unclamped level
    double R;           // dS_o / dnu
    double Fp, Fm;      // distance to the nearest kink above / below nu over the run that ends at o (INFINITY: none)
};

// LV (sto_cold_body): 1 (E0) the first tile is entered at the storage's initial level sto_e0(v)[s] (DOPF_F_STO_INITIAL_LEVEL), not at
// 0; 2 also classifies timestep T-1 against the terminal band [sto_end_lo, sto_end_hi] and roots it on lo or hi (DOPF_F_STO_TERMINAL_LEVEL);
// 3 (EF) as 2 with the level moving by be C - al D (DOPF_F_STO_EFFICIENCY): x_t, its slope and the kink distances dp / dm change
template <bool LINES, int LV = 0>
__global__ __launch_bounds__(kLongBS) void k_sto_long(DevView v)
{
    constexpr bool E0 = LV >= 1, EF = LV == 3;
    if (v.st->halt) return;
    __shared__ double wmap[3][kLongWaves];          // each wave's composite map of the tile
    __shared__ int wint[3][kLongWaves];             // candidate, last clamped step before it, last clamped step
    __shared__ double wdbl[7][kLongWaves];          // level at the candidate; slope / kinks up to it; slope / kinks after the last clamp
    __shared__ double redc[kLongBS];
    constexpr int NCH = kLongNCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x;
    const Item it = v.sto_items[blk];
    const int T = v.T, N = v.N;
    const double w = v.w_prox, gam = v.gamma, iw = 1.0 / w;
    const double a0 = w + gam, ia0 = 1.0 / a0, idet0 = 1.0 / (a0 * a0 - gam * gam), s20 = 2.0 / (a0 + gam);
    const int nTiles = (T + kLongTile - 1) / kLongTile;
    double accCost = 0.0;
    unsigned long long fails = 0;

    for (int s = it.a0; s < it.a1; ++s) {
        const double mc = v.sto_mc[s], pm = v.sto_pmax[s], em = v.sto_emax[s];
        const size_t row = (size_t)s * T;
        double *nuf = v.nu_prev + row;              // the price of each timestep, as the recursion assigns it
        const double tol = 1e-11 * (1.0 + em);
        const double e0 = E0 ? sto_e0(v)[s] : 0.0;   // level before timestep 0
        const double al = EF ? sto_eff_alpha(v)[s] : 1.0, be = EF ? sto_eff_beta(v)[s] : 1.0, ial = EF ? 1.0 / al : 1.0, ibe = EF ? 1.0 / be : 1.0;
        const double elo = LV >= 2 ? sto_end_lo(v)[s] : 0.0, ehi = LV >= 2 ? sto_end_hi(v)[s] : em;    // band of timestep T-1

        // the lane's inputs of timesteps tbase .. tbase + NCH - 1 (those > lim: zeros, never evaluated)
        double D0[NCH], C0[NCH], P0[NCH], K0[NCH];
        bool lin[NCH];
        auto load = [&](int tbase, int lim) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int t = tbase + c;
                const bool ok = t <= lim;
                D0[c] = ok ? v.D[row + t] : 0.0;
                C0[c] = ok ? v.C[row + t] : 0.0;
                P0[c] = 0.0; K0[c] = 0.0; lin[c] = false;
                if (!LINES) {
                    P0[c] = ok ? v.price[it.node + (size_t)N * t] + gam * v.s[t] : 0.0;
                } else if (ok) {
                    const size_t at = (size_t)it.node + (size_t)N * t;
                    const int m_ = v.tb_m[at];
                    const double p0_ = v.tb_psi0[at], k_ = v.tb_slope[at * (v.M2 + 1)];
                    if (m_ == 0) { lin[c] = true; P0[c] = p0_; K0[c] = k_; }
                }
            }
        };
        // x_t(nu) of lane step c = timestep t, as in sto_cold_body (the piece hint of a table starts at 0: it only saves probes)
        auto eval = [&](int c, int t, double nu, double &dd, double &cc, double &s1, double &pc) {
            const double nD = EF ? al * nu : nu, nC = EF ? be * nu : nu;      // the price as D's and as C's gradient see it
            if (!LINES) {
                const double q0 = D0[c] - C0[c], theta = P0[c] - gam * q0;
                box2(a0, gam, ia0, idet0, s20, w * D0[c] - mc - theta - nD, w * C0[c] - mc + theta + nC, pm, dd, cc, s1);
                if (EF) s1 = eff_slope(a0, gam, ia0, idet0, al, be, pm, dd, cc);
                pc = theta + gam * (dd - cc);
            } else if (lin[c]) {
                const double q0 = D0[c] - C0[c], theta = P0[c] - K0[c] * q0;
                double lia, lidet, ls2;
                lin_coef(w, iw, K0[c], lia, lidet, ls2);
                box2(w + K0[c], K0[c], lia, lidet, ls2, w * D0[c] - mc - theta - nD, w * C0[c] - mc + theta + nC, pm, dd, cc, s1);
                if (EF) s1 = eff_slope(w + K0[c], K0[c], lia, lidet, al, be, pm, dd, cc);
                pc = theta + K0[c] * (dd - cc);
            } else {
                const TabRef tb = tab_ref(v, it.node, t);
                int hint = 0;
                if constexpr (EF) eval_lines(tb, hint, w, iw, mc, pm, D0[c], C0[c], nu, al, be, dd, cc, s1, pc);
                else eval_lines(tb, hint, w, iw, mc, pm, D0[c], C0[c], nu, dd, cc, s1, pc);
            }
        };

        // One scan at price nu over the timesteps [0, lim]. Candidate: vv (root search, lim = vv) or the last timestep whose
        // unclamped level leaves the band (classification, lim = k).
        auto scan = [&](double nu, int lim, bool root, int vv) -> LongCand {
            LongCand cd{-1, 0.0, 0.0, INFINITY, INFINITY};
            double eT = e0;                                     // level entering the tile
            double cR = 0.0, cFp = INFINITY, cFm = INFINITY;    // slope / kinks since the last clamped step before the tile
            const int nt = lim / kLongTile + 1;
            for (int tb = 0; tb < nt; ++tb) {
                const int tbase = tb * kLongTile + tid * NCH;
                const int wbase = tb * kLongTile + wave * kLongWaveSteps;
                load(tbase, lim);
                double Sv[NCH], sg[NCH], dp[NCH], dm[NCH];
                Map3 loc;
                loc.A = 0.0; loc.LO = -INFINITY; loc.HI = INFINITY;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int t = tbase + c;
                    double dd = 0.0, cc = 0.0, s1 = 0.0, pc = 0.0;
                    dp[c] = INFINITY; dm[c] = INFINITY;
                    if (t <= lim) {
                        eval(c, t, nu, dd, cc, s1, pc);
                        // the four prices at which D or C would leave a bound (flat pieces: sto_cold_body's flat_jump)
                        const double bD = w * D0[c] - mc - pc, bC = mc - w * C0[c] - pc, wp = w * pm;
                        // (EF: D's two at b / al, C's two at b / be)
                        const double cand[4] = {EF ? bD * ial : bD, EF ? (bD - wp) * ial : bD - wp, EF ? bC * ibe : bC, EF ? (bC + wp) * ibe : bC + wp};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double d = cand[q] - nu;
                            if (d > 0.0) dp[c] = fmin(dp[c], d);
                            if (-d > 0.0) dm[c] = fmin(dm[c], -d);
                        }
                    }
                    Sv[c] = EF ? be * cc - al * dd : cc - dd;
                    sg[c] = s1;
                    loc.A += Sv[c];
                    loc.LO = clampd(loc.LO + Sv[c], 0.0, em);
                    loc.HI = clampd(loc.HI + Sv[c], 0.0, em);
                }
                Map3 inc = loc;
                scan_maps<64>(inc, (int)(threadIdx.x & 63));       // (the lane as the shared helpers' other callers pass it)
                Map3 ex;
                ex.A = prev_lane<64>(inc.A); ex.LO = prev_lane<64>(inc.LO); ex.HI = prev_lane<64>(inc.HI);
                if (lane == 63) { wmap[0][wave] = inc.A; wmap[1][wave] = inc.LO; wmap[2][wave] = inc.HI; }
                __syncthreads();
                double ew = eT;
                for (int w2 = 0; w2 < wave; ++w2) ew = clampd(ew + wmap[0][w2], wmap[1][w2], wmap[2][w2]);
                double eN = eT;
#pragma unroll
                for (int w2 = 0; w2 < kLongWaves; ++w2) eN = clampd(eN + wmap[0][w2], wmap[1][w2], wmap[2][w2]);
                double e = lane == 0 ? ew : clampd(ew + ex.A, ex.LO, ex.HI);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    Sv[c] = e + Sv[c];                          // unclamped level after timestep tbase + c
                    e = clampd(Sv[c], 0.0, em);
                }

                // the wave's candidate and the last clamped steps (before it; anywhere in the wave)
                int oW = -1, cB = -1, cA = -1;
                if (root) {
                    oW = (vv >= wbase && vv < wbase + kLongWaveSteps) ? vv - wbase : -1;
                } else {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const unsigned long long b = __ballot(tbase + c <= lim && (LV >= 2 && tbase + c == T - 1 ? (Sv[c] < elo - tol || Sv[c] > ehi + tol)
                                                                                                              : (Sv[c] < -tol || Sv[c] > em + tol)));
                        if (b) { const int j = (63 - __clzll(b)) * NCH + c; oW = j > oW ? j : oW; }
                    }
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int j = lane * NCH + c;
                    const bool cl = tbase + c <= lim && (Sv[c] <= 0.0 || Sv[c] >= em);
                    const unsigned long long bA = __ballot(cl), bB = __ballot(cl && j < oW);
                    if (bA) { const int q = (63 - __clzll(bA)) * NCH + c; cA = q > cA ? q : cA; }
                    if (bB) { const int q = (63 - __clzll(bB)) * NCH + c; cB = q > cB ? q : cB; }
                }
                double pO = 0.0, fpO = INFINITY, fmO = INFINITY, pA = 0.0, fpA = INFINITY, fmA = INFINITY, sel = 0.0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int j = lane * NCH + c;
                    if (j > cB && j <= oW) { pO += sg[c]; fpO = fmin(fpO, dp[c]); fmO = fmin(fmO, dm[c]); }
                    if (j > cA && tbase + c <= lim) { pA += sg[c]; fpA = fmin(fpA, dp[c]); fmA = fmin(fmA, dm[c]); }
                    if (j == oW) sel = Sv[c];
                }
                pO = group_sum<64>(pO); fpO = group_min<64>(fpO); fmO = group_min<64>(fmO);
                pA = group_sum<64>(pA); fpA = group_min<64>(fpA); fmA = group_min<64>(fmA);
                const double svO = oW >= 0 ? __shfl(sel, oW / NCH) : 0.0;
                if (lane == 0) {
                    wint[0][wave] = oW >= 0 ? wbase + oW : -1;
                    wint[1][wave] = cB >= 0 ? wbase + cB : -1;
                    wint[2][wave] = cA >= 0 ? wbase + cA : -1;
                    wdbl[0][wave] = svO; wdbl[1][wave] = pO; wdbl[2][wave] = fpO; wdbl[3][wave] = fmO;
                    wdbl[4][wave] = pA; wdbl[5][wave] = fpA; wdbl[6][wave] = fmA;
                }
                __syncthreads();
                // the tile's candidate (the last wave's, if any): its run goes back to the last clamped step, across waves and tiles
                int wo = -1;
#pragma unroll
                for (int w2 = 0; w2 < kLongWaves; ++w2) if (wint[0][w2] >= 0) wo = w2;
                if (wo >= 0) {
                    double R = wdbl[1][wo], Fp = wdbl[2][wo], Fm = wdbl[3][wo];
                    bool hit = wint[1][wo] >= 0;
                    for (int w2 = wo - 1; w2 >= 0 && !hit; --w2) {
                        R += wdbl[4][w2]; Fp = fmin(Fp, wdbl[5][w2]); Fm = fmin(Fm, wdbl[6][w2]);
                        hit = wint[2][w2] >= 0;
                    }
                    if (!hit) { R += cR; Fp = fmin(Fp, cFp); Fm = fmin(Fm, cFm); }
                    cd.o = wint[0][wo]; cd.sv = wdbl[0][wo]; cd.R = R; cd.Fp = Fp; cd.Fm = Fm;
                }
                {   // carry: slope / kinks since the last clamped step of the tiles scanned so far
                    double R = 0.0, Fp = INFINITY, Fm = INFINITY;
                    bool hit = false;
                    for (int w2 = kLongWaves - 1; w2 >= 0 && !hit; --w2) {
                        R += wdbl[4][w2]; Fp = fmin(Fp, wdbl[5][w2]); Fm = fmin(Fm, wdbl[6][w2]);
                        hit = wint[2][w2] >= 0;
                    }
                    if (!hit) { R += cR; Fp = fmin(Fp, cFp); Fm = fmin(Fm, cFm); }
                    cR = R; cFp = Fp; cFm = Fm;
                }
                eT = eN;
            }
            return cd;
        };

        // ---- price-threshold recursion, backwards over constant-price segments (sto_cold_body, block-uniform state) ----
        double nu = 0.0;
        int k = T - 1, mode = 0, vv = -1, rit = 0;
        double target = 0.0, lo = -INFINITY, hi = INFINITY, step = 1.0;
        while (k >= 0) {
            const LongCand cd = scan(nu, mode == 1 ? vv : k, mode == 1, vv);
            auto flat_jump = [&](double dir) -> double {
                const double best = dir > 0.0 ? cd.Fp : cd.Fm;
                if (best < INFINITY) return nu + dir * (best + 1e-9 * (1.0 + fabs(nu) + best));
                const double tr = nu + dir * step;
                step *= 4.0;
                return tr;
            };
            if (mode == 1) {
                const double res = cd.sv - target;
                if (res < 0.0) lo = nu; else hi = nu;
                bool conv = fabs(res) <= 1e-12 * (1.0 + em) || rit >= v.rootCap;
                double trial = nu;
                if (!conv) {
                    const double sl = cd.R;
                    const bool both = lo > -INFINITY && hi < INFINITY;
                    if (sl > 0.0) {
                        double r = __builtin_amdgcn_rcp(sl);
                        r = r * (2.0 - sl * r);
                        trial = nu - res * r;
                    } else {
                        trial = both ? 0.5 * (lo + hi) : flat_jump(res < 0.0 ? 1.0 : -1.0);
                    }
                    const bool forceBis = both && rit >= 6 && (rit & 1);
                    if (!(trial > lo && trial < hi) || forceBis) {
                        if (both) trial = 0.5 * (lo + hi);
                        else { trial = (res < 0.0) ? nu + step : nu - step; step *= 4.0; }
                    }
                    if (!(trial > lo && trial < hi)) conv = true;   // bracket is two adjacent doubles
                }
                if (conv) {
                    if (rit >= v.rootCap && fabs(res) > 1e-7 * (1.0 + em)) ++fails;
                    if (tid == 0) nuf[vv] = nu;
                    k = vv - 1;
                    mode = 0;                   // (the next scan classifies at this price)
                } else {
                    nu = trial;
                    ++rit;
                }
            } else {
                const int vnew = cd.o;
                for (int t = vnew + 1 + tid; t <= k; t += kLongBS) nuf[t] = nu;
                if (vnew < 0) {
                    k = -1;
                } else {
                    vv = vnew;
                    if (LV >= 2 && vnew == T - 1) target = cd.sv < elo ? elo : ehi;
                    else target = cd.sv < 0.0 ? 0.0 : em;
                    const double res = cd.sv - target;
                    lo = -INFINITY; hi = INFINITY;
                    if (res < 0.0) lo = nu; else hi = nu;
                    step = 1.0 + fabs(nu);
                    if (cd.R > 0.0) {
                        double r = __builtin_amdgcn_rcp(cd.R);
                        r = r * (2.0 - cd.R * r);
                        nu -= res * r;
                    } else {
                        nu = flat_jump(res < 0.0 ? 1.0 : -1.0);
                    }
                    mode = 1;
                    rit = 0;
                }
            }
        }
        __syncthreads();                                // every price of the row is in nu_prev

        // ---- final (D, C) at each timestep's price, outputs, the item's per-timestep sums ------------------------------
        for (int tb = 0; tb < nTiles; ++tb) {
            const int tbase = tb * kLongTile + tid * NCH;
            load(tbase, T - 1);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int t = tbase + c;
                if (t >= T) continue;
                const double nt_ = nuf[t];
                double Dn, Cn, s1, pc;
                eval(c, t, nt_, Dn, Cn, s1, pc);
                const size_t e = row + t;
                v.D[e] = Dn;
                v.C[e] = Cn;
                if (LINES && (v.keepDeltas || v.walk_any[t])) v.dltS[e] = (Dn - Cn) - (D0[c] - C0[c]);
                nuf[t] = LINES ? nt_ : nt_ + (P0[c] - gam * (D0[c] - C0[c]));     // (as the scan body leaves it)
                const double q = Dn - Cn;
                double *part = LINES ? &v.part_T[(size_t)t * v.rowsT + it.row] : &v.part_sinj[(size_t)blk * T + t];
                *part = s == it.a0 ? q : *part + q;
                accCost += mc * (Dn + Cn);
            }
        }
        if (tid == 0) v.nu_valid[s] = 1;
        __syncthreads();                                // (the next storage's recursion overwrites nothing of this one's)
    }

    redc[tid] = accCost;
    __syncthreads();
    for (int sft = kLongBS / 2; sft > 0; sft >>= 1) {
        if (tid < sft) redc[tid] += redc[tid + sft];
        __syncthreads();
    }
    if (tid == 0) {
        v.part_scost[blk] = redc[0];
        if (fails) atomicAdd(&v.st->solver_fail, fails);
    }
}

}  // namespace dopf
