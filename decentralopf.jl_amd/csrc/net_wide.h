// net_wide.h — the consensus kernels of networks beyond 2048 lines (DOPF_F_WIDE_NETWORK; DOPF_F_DEBUG_WIDE_NET at any L > 0).
// Included by kernels_consensus.hip (uses its helpers: block_sum256, slack_case, slack_sum_cases, atomic_max_pos, ...).
//
// The rule of this chain: no LDS buffer grows with N or L. What the kernels of L <= 2048 stage whole is staged in chunks or read
// from memory, and the agent kernels read the same table layout (stride 2L) as before:
//   k_tables_wide   one 256-thread block per (n,t): build_table's classification over the 2L candidates in tiles of 1024 with the
//                   loads in flight; the survivors compacted in list order into LDS up to kWideCap entries, beyond that into the
//                   (n,t)'s own output rows (free scratch until the table is written). Runs of kWideCap are rank-sorted in LDS and
//                   merged pairwise in the rows (an element's place = its place in its run + a binary search in the other run);
//                   the order is (key, list position), a strict total order, so the result is build_table's order. Slopes and Psi
//                   are block scans with carries. The jump of a kink is recomputed from its candidate index (same expression, same
//                   bits), so a sort entry is one key and one int.
//   k_dual_tw       k_dual_t with the timestep's injections staged in chunks of kWideChunk nodes (same order of every sum)
//   k_price_tw      k_price_t with (mu - rho), G and S streamed in chunks of kWideChunk lines, and one block per (timestep, 256
//                   nodes); keeps walk_any, tab_skip and the linear Psi(0) / slope of a timestep without flagged lines
//   k_lines_wide    k_reduce's line-sum blocks with the node changes, windows and agent counts read from memory
// Every sum has a fixed order: two runs give the same bits.
#pragma once

namespace dopf {

constexpr int kWideCap = 128;           // table entries k_tables_wide keeps in LDS (one sorted run; typical tables have a handful)
constexpr int kWideChunk = 1024;        // nodes / lines per staged chunk of the dual and price kernels

// inclusive prefix sum over the block's 256 threads (Hillis-Steele in LDS: a fixed order); *total = the sum of all 256
__device__ __forceinline__ double block_scan256(double x, double *sh, double *total)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = x;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const double y = tid >= d ? sh[tid - d] : 0.0;
        __syncthreads();
        if (tid >= d) sh[tid] = y + sh[tid];
        __syncthreads();
    }
    const double r = sh[tid];
    *total = sh[255];
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool wide_before(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// the slope jump of candidate i (build_table's expressions)
__device__ __forceinline__ double wide_jump(const DevView &v, int n, int i, double w2, double act)
{
    const double h = v.ptdf[(i >> 1) + v.L * n];
    const double dj = w2 * h * h * (1.0 - act);
    return (i & 1) == 0 ? (h > 0.0 ? dj : -dj) : (h > 0.0 ? -dj : dj);
}

__global__ __launch_bounds__(256) void k_tables_wide(DevView v)
{
    if (v.st->halt) return;
    const size_t at = blockIdx.x;
    const int N = v.N, L = v.L, M2 = v.M2;
    const int n = (int)(at % N), t = (int)(at / N);
    if (v.tab_skip[t]) return;               // linear inside every window: the price kernel wrote Psi(0) and the slope
    __shared__ double lk[kWideCap];
    __shared__ int li[kWideCap];
    __shared__ double red[256];
    __shared__ int wc[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double w2 = 2.0 * v.w_flow, g = v.gamma, act = g / (w2 + g);
    const double W = v.node_win[n];
    // the rows of (n,t); until the table is written they hold two sort buffers: F = keys in ob, indices in opi[0, c),
    // S = keys in os[0, c), indices in opi[M2, M2 + c) (opi: the psi row as 2 * M2 ints)
    double *ob = v.tb_beta + at * M2, *op = v.tb_psi + at * M2, *os = v.tb_slope + at * (M2 + 1);
    int *opi = reinterpret_cast<int *>(op);

    // ---- classify the 2L candidate kinks (build_table's arithmetic); keep the ones inside [-W, W] in list order
    double s0part = 0.0, left = 0.0, pz = 0.0, nneg = 0.0;
    int c = 0;
    for (int base = 0; base < M2; base += 256 * 4) {        // four candidates per thread, their loads issued together
        double hh[4], ff[4], FF[4], au[4], ak[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + 256 * u + tid;
            const int l = (i < M2 ? i : 0) >> 1;
            hh[u] = v.ptdf[l + L * n]; ff[u] = v.flow[l + L * t]; FF[u] = v.fmax[l + v.fmax_ld * t];
            au[u] = v.avgU[l + L * t]; ak[u] = v.avgK[l + L * t];
        }
        double kvs[4];
        bool ins[4];
        unsigned long long mk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + 256 * u + tid;
            double kv = INFINITY, jv = 0.0;
            if (i < M2) {
                const double h = hh[u];
                if (h != 0.0) {
                    const double f = ff[u], F = FF[u];
                    const double dj = w2 * h * h * (1.0 - act);
                    if ((i & 1) == 0) {          // U switches: active where h*dlt < ...
                        kv = (g * au[u] / w2 - f + F) / h;
                        jv = h > 0.0 ? dj : -dj;
                        s0part += w2 * h * h * (1.0 + act);     // at -inf exactly one of U, K is active
                        const double U = dmax0((g * au[u] - w2 * (f - F)) / (w2 + g));
                        const double K = dmax0((g * ak[u] + w2 * (f + F)) / (w2 + g));
                        pz += w2 * h * ((f + U - F) - (K - f - F));
                    } else {                     // K switches
                        kv = (-g * ak[u] / w2 - f - F) / h;
                        jv = h > 0.0 ? -dj : dj;
                    }
                }
            }
            const bool fin = kv < INFINITY;                      // (also false for NaN)
            if (fin && kv < -W) left += jv;
            ins[u] = fin && kv >= -W && kv <= W;
            if (ins[u] && kv < 0.0) nneg += 1.0;
            kvs[u] = kv;
            mk[u] = __ballot(ins[u]);
            if (lane == 0) wc[u * 4 + wv] = (int)__popcll(mk[u]);
        }
        __syncthreads();
        int off[4], tot = 0;                                     // list order: u-th quarter of the tile, then wave, then lane
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            for (int w = 0; w < 4; ++w) {
                if (w == wv) off[u] = c + tot;
                tot += wc[u * 4 + w];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (ins[u]) {
                const int pos = off[u] + (int)__popcll(mk[u] & ((1ull << lane) - 1ull));
                const int i = base + 256 * u + tid;
                if (pos < kWideCap) { lk[pos] = kvs[u]; li[pos] = i; }
                else { os[pos] = kvs[u]; opi[M2 + pos] = i; }            // spilled into buffer S at its list position
            }
        }
        c += tot;
        __syncthreads();                                         // (wc is rewritten by the next tile)
    }
    const double slope_left = g + block_sum256(s0part, red) + block_sum256(left, red);    // slope just right of -W
    const double psiZ = v.price[n + N * t] + g * v.s[t] + block_sum256(pz, red);
    const int j0 = (int)block_sum256(nneg, red);                 // kept kinks < 0: 0 lies on piece j0

    // ---- sort by (key, list position): runs of kWideCap rank-sorted in LDS, then pairwise merges; the last pass writes F
    int passes = 0;
    for (int w = kWideCap; w < c; w <<= 1) ++passes;
    double *srcK = (passes & 1) ? os : ob, *dstK = (passes & 1) ? ob : os;
    int *srcI = (passes & 1) ? opi + M2 : opi, *dstI = (passes & 1) ? opi : opi + M2;
    for (int r0 = 0; r0 < c; r0 += kWideCap) {
        const int rn = min(kWideCap, c - r0);
        if (r0 > 0) {                                            // a spilled run: from buffer S into LDS (the first one is there)
            for (int e = tid; e < rn; e += 256) { lk[e] = os[r0 + e]; li[e] = opi[M2 + r0 + e]; }
            __syncthreads();
        }
        for (int e = tid; e < rn; e += 256) {
            const double ke = lk[e];
            int r = 0;
            for (int k = 0; k < rn; ++k) {
                const double kk = lk[k];
                r += (kk < ke || (kk == ke && k < e)) ? 1 : 0;
            }
            srcK[r0 + r] = ke;
            srcI[r0 + r] = li[e];
        }
        __syncthreads();
    }
    for (int w = kWideCap; w < c; w <<= 1) {
        for (int p = tid; p < c; p += 256) {
            const int a = (p / (2 * w)) * (2 * w), mid = min(a + w, c), e = min(a + 2 * w, c);
            const double k = srcK[p];
            const int id = srcI[p];
            const bool inLeft = p < mid;
            int lo = inLeft ? mid : a, hi = inLeft ? e : mid;    // count the other run's entries before (k, id)
            const int o0 = lo;
            while (lo < hi) {
                const int m = (lo + hi) >> 1;
                if (wide_before(srcK[m], srcI[m], k, id)) lo = m + 1;
                else hi = m;
            }
            const int q = a + (inLeft ? p - a : p - mid) + (lo - o0);
            dstK[q] = k;
            dstI[q] = id;
        }
        __syncthreads();
        double *tk = srcK; srcK = dstK; dstK = tk;
        int *ti = srcI; srcI = dstI; dstI = ti;
    }
    // (sorted: keys in ob, list positions in opi[0, c))

    // ---- slopes: piece 0 = left of the first kept kink, os[j + 1] = slope on piece j + 1 = right of kink j
    {
        double carry = slope_left;
        for (int b = 0; b < c; b += 256) {
            const int j = b + tid;
            const double jv = j < c ? wide_jump(v, n, opi[j], w2, act) : 0.0;
            double tot;
            const double pre = block_scan256(jv, red, &tot);
            if (j < c) os[j + 1] = carry + pre;
            carry += tot;
        }
    }
    __syncthreads();
    // ---- Psi at the kinks, outwards from 0 (the psi row's indices are consumed: it is written now)
    const double slope_j0 = j0 == 0 ? slope_left : os[j0];
    if (j0 < c) {                                                // right of 0: kinks j0, j0 + 1, ...
        double base = psiZ + slope_j0 * ob[j0];
        for (int b = j0; b < c; b += 256) {
            const int j = b + tid;
            const double d = (j < c && j > j0) ? os[j] * (ob[j] - ob[j - 1]) : 0.0;
            double tot;
            const double pre = block_scan256(d, red, &tot);
            if (j < c) op[j] = base + pre;
            base += tot;
        }
    }
    if (j0 > 0) {                                                // left of 0: kinks j0 - 1, j0 - 2, ...
        double base = psiZ + slope_j0 * ob[j0 - 1];
        for (int b = 0; b < j0; b += 256) {
            const int o = b + tid, j = j0 - 1 - o;
            const double d = (o < j0 && o > 0) ? os[j + 1] * (ob[j + 1] - ob[j]) : 0.0;
            double tot;
            const double pre = block_scan256(d, red, &tot);
            if (o < j0) op[j] = base - pre;
            base -= tot;
        }
    }
    if (tid == 0) {
        os[0] = slope_left;
        v.tb_m[at] = c;
        v.tb_psi0[at] = psiZ;
    }
}

// k_dual_t with the injections of the timestep staged kWideChunk nodes at a time. Thread (part, line) walks its part's nodes in
// order across the chunks and the imbalance adds node tid, tid + 256, ...: k_dual_t's orders.
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_dual_tw(DevView v)
{
    if (UPDATE && v.st->halt) return;
    __shared__ double q[kWideChunk];
    __shared__ double red[256];
    const int LB = (v.L + 63) / 64;
    const int tid = threadIdx.x, t = blockIdx.x / LB, lb = blockIdx.x - t * LB;
    const int N = v.N, L = v.L;
    const size_t NT = (size_t)N * v.T, LT = (size_t)L * v.T;
    const double *cinj = v.cons, *cU = v.cons + NT, *cK = cU + LT;
    const int pr = tid >> 6, ll = tid & 63, l = lb * 64 + ll;
    const int Nc = (((N + 3) / 4) + 7) & ~7, nbeg = pr * Nc, nend = min(N, nbeg + Nc);
    double part = 0.0, f = 0.0;
    for (int c0 = 0; c0 < N; c0 += kWideChunk) {
        const int c1 = min(N, c0 + kWideChunk);
        __syncthreads();                                         // (the previous chunk is consumed)
        for (int n = c0 + tid; n < c1; n += 256) {
            const double x = cinj[n + (size_t)N * t] - v.demand[n + (size_t)N * t];
            q[n - c0] = x;
            if (lb == 0) v.inj[n + (size_t)N * t] = x;                    // results.jl:58-100
            part += x;
        }
        __syncthreads();
        const int a = max(nbeg, c0), b = min(nend, c1);
        if (l < L)
            for (int n0 = a; n0 < b; n0 += 8) {                           // eight rows of ptdf in flight
                double h[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) h[u] = n0 + u < b ? v.ptdf[l + (size_t)L * (n0 + u)] : 0.0;
#pragma unroll
                for (int u = 0; u < 8; ++u) f += h[u] * (n0 + u < b ? q[n0 + u - c0] : 0.0);
            }
    }
    const double sum = block_sum256(part, red);
    double rl = 0.0, rm = 0.0, rr = 0.0;
    if (tid == 0 && lb == 0) {
        if (UPDATE) v.s_used[t] = v.s[t];
        v.s[t] = sum;
        if (UPDATE) {
            const double lo = v.lam[t], ln = lo + v.gamma * sum;             // update_duals.jl:8-13
            v.lam_used[t] = lo;
            v.lam[t] = ln;
            rl = fabs(ln - lo);
        }
    }
    __syncthreads();
    red[tid] = f;
    __syncthreads();
    if (pr == 0 && l < L) {
        f = ((red[ll] + red[64 + ll]) + red[128 + ll]) + red[192 + ll];
        const size_t i = l + (size_t)L * t;
        if (UPDATE) { v.flow_used[i] = v.flow[i]; v.avgU_used[i] = v.avgU[i]; v.avgK_used[i] = v.avgK[i]; }
        v.flow[i] = f;                                                       // results.jl:114
        if (UPDATE) {
            const double aU = v.invA * cU[i], aK = v.invA * cK[i];          // results.jl:108-112
            v.avgU[i] = aU;
            v.avgK[i] = aK;
            const double mo = v.mu[i], ro = v.rho[i], F = v.fmax[l + v.fmax_ld * t];
            const double mn = (mo + v.gamma * (f + aU - F)) * (aU <= v.mask_thr ? 1.0 : 0.0);   // update_duals.jl:18-25
            const double rn = (ro + v.gamma * (aK - f - F)) * (aK <= v.mask_thr ? 1.0 : 0.0);   // :30-37
            v.mu_used[i] = mo; v.rho_used[i] = ro;
            v.mu[i] = mn; v.rho[i] = rn;
            rm = fabs(mn - mo);
            rr = fabs(rn - ro);
        }
        const double w2 = 2.0 * v.w_flow, inv = 1.0 / (w2 + v.gamma);
        v.walk_flag[i] = slack_needs_cases(v.gamma, w2, inv, f, v.fmax[l + v.fmax_ld * t], v.avgU[i], v.avgK[i], v.line_reach[l]) ? 1 : 0;
    }
    if (UPDATE) {
        __syncthreads();
        red[tid] = rm;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] = fmax(red[tid], red[tid + s]); __syncthreads(); }
        const double bm = red[0];
        __syncthreads();
        red[tid] = rr;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] = fmax(red[tid], red[tid + s]); __syncthreads(); }
        if (tid == 0) {
            if (rl > 0.0) atomic_max_pos(&v.st->resbits[0], rl);
            if (bm > 0.0) atomic_max_pos(&v.st->resbits[1], bm);
            if (red[0] > 0.0) atomic_max_pos(&v.st->resbits[2], red[0]);
            if (t == 0 && lb == 0) v.st->total_cost = v.cons[NT + 2 * LT];
        }
    }
}

// k_price_t for any L: block (timestep t, batch of up to 256 nodes); (mu - rho), G and S of the timestep's lines pass through LDS
// kWideChunk lines at a time. Thread (part, n) adds its part's lines in order across the chunks, the parts meet in part order.
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_price_tw(DevView v)
{
    __shared__ double d[kWideChunk], Gl[kWideChunk], Sl[kWideChunk];
    __shared__ double redp[3][256];
    const int N = v.N, L = v.L;
    const int NP = N <= 256 ? ((N + 31) & ~31) : 256, P = 256 / NP, NB = (N + NP - 1) / NP;
    const int tid = threadIdx.x, t = blockIdx.x / NB, nb = (blockIdx.x - t * NB) * NP;
    int anyNeed = 0, nz = 0;
    for (int l = tid; l < L; l += 256) {
        const size_t i = l + (size_t)L * t;
        anyNeed |= v.walk_flag[i];
        nz |= (v.mu[i] - v.rho[i]) != 0.0;
    }
    anyNeed = __syncthreads_or(anyNeed);
    nz = __syncthreads_or(nz);
    if (tid == 0 && nb == 0 && L > 0) v.walk_any[t] = anyNeed ? 1 : 0;
    const bool lin = L > 0 && !anyNeed;
    const double w2 = 2.0 * v.w_flow, g = v.gamma, inv = 1.0 / (w2 + g);
    const double lam = v.lam[t], gs = g * v.s[t];
    const int part = tid / NP, nn = tid - part * NP;
    const int Lc = (((L + P - 1) / P) + 7) & ~7, lbeg = part * Lc, lend = min(L, lbeg + Lc);
    const int n = nb + nn;
    double p = 0.0, ps = 0.0, sl = 0.0;
    if (nz || lin)
        for (int c0 = 0; c0 < L; c0 += kWideChunk) {
            const int c1 = min(L, c0 + kWideChunk);
            __syncthreads();                                     // (the previous chunk is consumed)
            for (int l = c0 + tid; l < c1; l += 256) {
                const size_t i = l + (size_t)L * t;
                d[l - c0] = v.mu[i] - v.rho[i];
                if (lin) {
                    const double f = v.flow[i], F = v.fmax[l + v.fmax_ld * t];
                    const double U0 = dmax0((g * v.avgU[i] - w2 * (f - F)) * inv), K0 = dmax0((g * v.avgK[i] + w2 * (f + F)) * inv);
                    Gl[l - c0] = w2 * ((f + U0 - F) - (K0 - f - F));
                    Sl[l - c0] = w2 * (2.0 - ((U0 > 0.0 ? 1.0 : 0.0) + (K0 > 0.0 ? 1.0 : 0.0)) * w2 * inv);
                }
            }
            __syncthreads();
            const int a = max(lbeg, c0), b = min(lend, c1);
            if (n < N && part < P)
                for (int l0 = a; l0 < b; l0 += 8) {                          // ptdfT[n + N l]: coalesced over the nodes
                    double h[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) h[u] = l0 + u < b ? v.ptdfT[n + (size_t)N * (l0 + u)] : 0.0;
#pragma unroll
                    for (int u = 0; u < 8; ++u) p += h[u] * (l0 + u < b ? d[l0 + u - c0] : 0.0);
                    if (lin) {
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (l0 + u < b) { ps += h[u] * Gl[l0 + u - c0]; sl += h[u] * h[u] * Sl[l0 + u - c0]; }
                    }
                }
        }
    if (P > 1) {
        __syncthreads();
        redp[0][tid] = p; redp[1][tid] = ps; redp[2][tid] = sl;
        __syncthreads();
        if (part == 0)
            for (int k = 1; k < P; ++k) { p += redp[0][k * NP + nn]; ps += redp[1][k * NP + nn]; sl += redp[2][k * NP + nn]; }
    }
    if (n < N && part == 0) {
        const size_t at = n + (size_t)N * t;
        p += lam;
        v.price[at] = p;
        if (lin) {
            v.tb_m[at] = 0;
            v.tb_psi0[at] = (p + gs) + ps;
            v.tb_slope[at * (v.M2 + 1)] = g + sl;
        }
    }
    if (L > 0 && tid == 0 && nb == 0) v.tab_skip[t] = lin ? 1 : 0;
    if (UPDATE && t == 0 && nb == 0 && tid == 0) {
        Status *st = v.st;
        if (st->halt) return;
        const double r0 = __longlong_as_double((long long)st->resbits[0]);
        const double r1 = __longlong_as_double((long long)st->resbits[1]);
        const double r2 = __longlong_as_double((long long)st->resbits[2]);
        st->resbits[0] = st->resbits[1] = st->resbits[2] = 0ull;
        status_update(v, r0, r1, r2);
    }
}

// k_reduce's line-sum blocks (same grid mapping and arithmetic) with the nodes' changes, windows and agent counts read from
// memory instead of LDS: block (timestep, U | K, group of 64 lines), thread (node part, line)
__global__ __launch_bounds__(256) void k_lines_wide(DevView v)
{
    if (v.st->halt) return;
    __shared__ double pred[256];
    const int tid = threadIdx.x;
    const int N = v.N, L = v.L, T = v.T;
    const double *sdL = v.node_dsum, *winL = v.node_win, *naL = v.node_na;
    const int LB = (L + 63) / 64;
    const int lb = blockIdx.x % LB, tw = blockIdx.x / LB, t = tw >> 1, which = tw & 1;
    sdL += (size_t)N * t;
    const int pr = tid >> 6, ll = tid & 63, l = lb * 64 + ll;
    const int Nc = (((N + 3) / 4) + 7) & ~7, nbeg = pr * Nc, nend = min(N, nbeg + Nc);
    const double w2 = 2.0 * v.w_flow, g = v.gamma, inv = 1.0 / (w2 + g);
    double partial = 0.0;
    if (l < L && nbeg < nend) {
        const size_t rem = l + (size_t)L * t;
        const double f = v.flow[rem], F = v.fmax[l + v.fmax_ld * t], cu = v.avgU[rem], ck = v.avgK[rem];
        if (!v.walk_flag[rem]) {
            const SlackCase c0 = slack_case(g, w2, inv, 0.0, f, F, cu, ck, 0.0);
            const double a = which ? c0.aK : c0.aU;
            if (a > 0.0) {
                double dot = 0.0, cnt = 0.0;
                for (int n0 = nbeg; n0 < nend; n0 += kFlight) {
                    double h[kFlight];
#pragma unroll
                    for (int u = 0; u < kFlight; ++u) h[u] = n0 + u < nend ? v.ptdf[l + (size_t)L * (n0 + u)] : 0.0;
#pragma unroll
                    for (int u = 0; u < kFlight; ++u)
                        if (n0 + u < nend) { dot = fma(h[u], sdL[n0 + u], dot); cnt += naL[n0 + u]; }
                }
                partial = slack_sum_plain(which, cnt, a, w2 * inv, dot);
            }
        } else {
            partial = slack_sum_cases(v, which, l, t, nbeg, nend, sdL, winL, naL, f, F, cu, ck);
        }
    }
    pred[tid] = partial;
    __syncthreads();
    if (pr == 0 && l < L)
        v.cons[(size_t)N * T + (size_t)which * L * T + l + (size_t)L * t] = ((pred[ll] + pred[64 + ll]) + pred[128 + ll]) + pred[192 + ll];
}

void launch_tables_wide(const DevView &v, hipStream_t s)
{
    hipLaunchKernelGGL(k_tables_wide, dim3((unsigned)((size_t)v.N * v.T)), dim3(256), 0, s, v);
}

// k_reduce's node blocks alone (its line blocks are not in the grid: no LDS), then the line sums
void launch_reduce_wide(const DevView &v, hipStream_t s)
{
    const int TC = (v.T + 31) / 32;
    hipLaunchKernelGGL(k_reduce, dim3(v.N * v.reduceRB * TC), dim3(256), 0, s, v);
    hipLaunchKernelGGL(k_lines_wide, dim3(2 * v.T * ((v.L + 63) / 64)), dim3(256), 0, s, v);
}

template <bool UPDATE>
inline void launch_dual_wide(const DevView &v, hipStream_t s)
{
    const int NP = v.N <= 256 ? ((v.N + 31) & ~31) : 256, NB = (v.N + NP - 1) / NP;
    hipLaunchKernelGGL(k_dual_tw<UPDATE>, dim3(v.T * ((v.L + 63) / 64)), dim3(256), 0, s, v);
    hipLaunchKernelGGL(k_price_tw<UPDATE>, dim3(v.T * NB), dim3(256), 0, s, v);
}

}  // namespace dopf
