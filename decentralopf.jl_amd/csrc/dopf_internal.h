// dopf_internal.h — shared declarations of libdopf_hip (gfx950 only).
//
// Layout of everything that lives in HBM (all fp64 unless noted):
//   P            [t + T*g]      generator output, updated IN PLACE each iteration (the x-update of a
//                               generator needs only its own previous value), generators sorted by node
//   D, C         [t + T*s]      storage discharge / charge, in place, storages sorted by node
//   E            [t + T*s]      storage level = cumsum(C - D): written on request only (dopf_get_primal, the central solver)
//   dltG, dltS   [t + T*a]      change of the agent's net injection in this iteration (only when L > 0:
//                               feeds the slack sums sum_a U_a, sum_a K_a)
//   lam [T], mu/rho [l + L*t]   current duals; *_used = the ones the last solve read
//   inj [n + N*t], s [T], flow [l + L*t], avgU/avgK [l + L*t], price [n + N*t]
//                               consensus state of the previous iteration, replicated per GPU
//   tb_*         per (n,t) breakpoint tables of Psi_{n,t} (only when L > 0)
//   part_*       per work-item partial sums, reduced in a fixed order (bitwise reproducible)
//   cons         [N*T | L*T | L*T | 1]  the consensus vector that is all-reduced across ranks
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/dopf.h"
#include "dopf_plan.h"
#include "ramp_dp.h"
#include "budget_root.h"
#include "ramp_budget.h"
#include "central_rows.h"

namespace dopf {

// device-resident status word block (one per context)
struct Status {
    int iteration;          // admm.iteration (1-based)
    int converged;          // Convergence.all
    int halt;               // converged || iteration > max_iters: every kernel returns at once
    int iters_total;        // iterations computed since creation
    unsigned long long solver_fail;
    unsigned long long dbg_scans, dbg_wave_loops, dbg_events;   // storage kernel statistics (DOPF_STATS builds)
    unsigned long long dbg_cyc[6];                              // DOPF_STATS: wave cycles per section of the storage body
    unsigned long long dbg_reason[4];                           // DOPF_STATS: no prices / Newton / level / sign
    unsigned long long resbits[3];   // running max of |dual change| as bit patterns (>= 0 doubles)
    unsigned long long resbits2[2][3];   // k_dual_price_t1024: the same, one set per iteration parity (the stop test does not read them:
                                         // its ticket word carries "some residual >= eps"); the host decodes the reported set
    int walk_last;                  // k_dual_price_t1024: timesteps for which the last dual step flagged a line (k_slack has agents to walk in the next iteration)
    int res_set;                    // -1: res[] holds the residuals of the last checked iteration; 0/1: resbits2[res_set] does
    double res[3];          // lambda / mu / rho residual inf-norms of the last checked iteration
    double total_cost;
    int xchg_timeout;       // peer exchange: a peer's part of the consensus sum did not arrive in time (sticky)
    int tail_timeout;       // tail in the launch: the block sums of an iteration did not all arrive in time (sticky)
    int tail_par;           // tail in the launch: which of the two accumulator sets the next launch adds into
};

struct XchgView;
// accumulators of the one-launch iterations (kernels_agents.hip); lives in device memory
struct TailView {
    long long *acc;                 // [2 sets][kAccRep][accStride]: slots 0..T-1 injection sums, slot T cost
    int accStride;
    int expect;                     // blocks that add to every slot (generator blocks + storage items)
    double scaleInj, invInj, scaleCost, invCost;        // fixed-point scales (powers of two) and their inverses
    const XchgView *xchg;           // non-null (a context joined to a peer exchange): the tail block sums its vector over the ranks
                                    // itself, between its own sums and the dual step (device copy of the exchange's view)
};

struct DevView {
    const DevView *self;            // this view in device memory (what a non-inlined device function is handed)
    int N, L, T, G, S, M2;          // M2 = 2L
    int maxNodeAgents;              // most agents (generators + storages) at one node
    int nGenItems, nStoItems;
    int genTT, genR;                // generator block tiling: TT = min(T, 512) timesteps x R agents
    int genRows;                    // > 0: (one node) the generators' partial sums are this many rows, one per streaming block, not one per item
    int genBlocks;                  // > 0 (needs genChunk): the fused launch has this many generator blocks, each walking items b, b + genBlocks, ...
    int debugLeave;                 // DOPF_F_DEBUG_LEAVE (tests)
    double *part_T;                 // networks (L > 0): the items' partial injection sums TRANSPOSED, [t][row] with rowsT rows per timestep — node by node
    int rowsT;                      // (a node's generator items, then two rows per storage item: scan partial, warm-start partial). The block of the
                                    // dual/price kernel that owns timestep t reads ALL rows of t as one contiguous vector (the quiet chain: no k_slack
                                    // launch) instead of one 8-byte word out of every row of the [row][t] layout the copper plates keep (part_*inj);
                                    // the sums are formed in the same order from either layout: same bits. Null: part_ginj / part_sinj / part_sinj_w.
    int rowsN;                      // ... of which rowsN are items' rows: the rows are PLACED by the XCD their writer block runs on (block index mod 8,
    const int *row_of_pos, *pos_of_row;   // eight regions on 128-byte boundaries) — written in node order, every 128-byte line of a timestep would collect 8-byte
                                    // pieces in all eight L2s and be written back eight times at the kernel's end. row_of_pos[p]: the node-ordered row
                                    // at position p (-1: padding); pos_of_row: its inverse. Item::row is a POSITION.
    int dualRowsOff, dualSdOff;     // the one-launch dual/price kernel's dynamic LDS, in doubles: where the rows of its timestep (aliased with the tables'
    int dualLdsBytes;               // scratch) and the vectors behind them start, and its size
    int tablesInDual;               // > 0 (networks on the one-launch dual/price kernel): that kernel builds the breakpoint tables of its
                                    // timestep itself, with this many waves; no k_tables launch
    int stoChunk;                   // > 0: one node, storage item i = storages [i*stoChunk, (i+1)*stoChunk)
    int genChunk;                   // > 0: one node, generator item i = rows [i*genChunk, (i+1)*genChunk) (no item look-up)
    int genSkip;                    // pair kernel with row skipping (blocks sweep >= 8 passes of agents)
    int genTT2, genR2;              // pair kernel (copper plate, even T <= 1024): T/2 double2 columns x R2 agents; 0 = off
    int sliceDual;                  // per launch: k_reduce stops after the slice sums (level 1) and the one-block dual
                                    // kernel adds the slices itself (single-GPU iterate path, small consensus state)
    int reduceRB;                   // reduce blocks per node (two-level fixed-order sum)
    int slackInDual;                // per launch (networks on the one-launch dual/price kernel, single-GPU chain): k_slack stores the node
                                    // sums and the cost itself, the dual/price block of timestep t forms the slack sums of its lines from the
                                    // PTDF rows it reads anyway — no k_reduce launch
    int slackGlobal;                // per launch (contexts on a peer exchange, no line flagged): the chain of slackInDual with the exchange of
                                    // the node sums between k_slack and the dual/price kernel — that kernel then takes the nodes' injection
                                    // changes from the SUMMED injections (this iteration's minus the previous one's, both replicated) and counts
                                    // all ranks' agents; a dual step that flags a line parks the chain (as the quiet chain does)
    int quiet;                      // per launch (with slackInDual): the quiet chain — no line is flagged, k_slack is not launched, the dual/price
                                    // kernel forms the node sums too
    int genTT256;                   // networks, fused launch: column tiling of a 256-thread generator block with the same R as genR
    int use_warm;                   // storage warm-start kernel runs first; the scan kernel serves its failures
    int max_iters;
    int keepDeltas;                 // DOPF_F_KEEP_DELTAS: dltG / dltS are written for every timestep (diagnostic getters)
    int rootCap;                    // iteration cap of the scan kernel's root search (80; 2 with DOPF_F_DEBUG_ROOT_CAP)
    int fmax_ld;                    // the line limit of (l,t) is fmax[l + fmax_ld * t]: 0 (one limit per line), L with DOPF_F_LINE_RATING (the
                                    // rating table). It sits in what was padding in front of gamma: the view keeps its size and every offset
    double gamma, w_flow, w_prox, eps, mask_thr, invA;
    double nAgents;                 // the divisor of avg_U / avg_K as a number: all ranks' agents (1 / invA without the rounding)
    double cp_ia, cp_idet, cp_s2;   // copper-plate box2 constants with a = w_prox + gamma, b = gamma: 1/a, 1/(a^2 - b^2), 2/(a + b) (host: no divisions per block)
    // problem (read-only)
    const double *demand, *ptdf, *fmax;             // fmax: [l + fmax_ld*t] (DOPF_F_LINE_RATING: the L x T rating table, then dopf_create's L limits)
    const double *ptdfT;                            // [n + N*l]: the transpose, for the price kernel's node-major threads
    const double *gen_mc, *gen_pmax;                // DOPF_F_GEN_QUADRATIC_COST: gen_mc has 2G entries, the quadratic coefficients behind the costs (gen_c2(v))
                                                    // DOPF_F_GEN_RAMP: the ramps, the anchor and k_gen_ramp's scratch behind gen_pmax (gen_ramp_up(v) ..)
    const double2 *gen_mp;                          // [g] {mc, pmax} side by side: one 16-byte load per row (streaming blocks)
    const double *sto_mc, *sto_pmax, *sto_emax;     // DOPF_F_STO_INITIAL_LEVEL: sto_emax has 2S entries, the initial levels behind the max levels
                                                    // (sto_e0(v) below): the view, every kernel's argument, keeps its layout;
                                                    // DOPF_F_STO_TERMINAL_LEVEL: 4S, the terminal bands behind those (sto_end_lo/hi)
    const Item *gen_items, *sto_items;
    const int *node_gen_beg, *node_sto_beg;         // N+1 each: agent ranges per node
    const double *node_win;                         // N: bound on |change of an agent's net injection| at the node
    const int *node_gitem_beg, *node_sitem_beg;     // N+1 each: item ranges per node
    // primal state
    double *P, *D, *C, *E, *dltG, *dltS;
    int *gen_state;                 // per generator: 0 = P all zero, 1 = all at pmax, 2 = mixed (pair kernel's row skipping)
    // duals and consensus state
    double *lam, *mu, *rho, *lam_used, *mu_used, *rho_used;
    double *inj, *s, *flow, *avgU, *avgK, *price;
    double *s_used, *flow_used, *avgU_used, *avgK_used;   // what the last x-update read (diagnostic getters: per-agent U, K, penalty terms)
    // tables
    double *tb_beta, *tb_psi, *tb_slope, *tb_psi0;
    int *tb_m;
    // partials
    double *part_ginj, *part_gcost;                 // [item*T + t], [item]
    double *part_sinj, *part_scost;                 // storage scan kernel, per item
    double *part_sinj_w, *part_scost_w;             // storage warm-start kernel, per item
    double *nu_prev;                                // [t + T*s] price of stored energy of the last solve (copper plates: + the step's price offset theta)
    int *nu_valid, *sto_fail, *item_fail;           // [s], [s], [item] (= storages of the item the warm start left over)
    double *part_U, *part_K;                        // [(n + N*t)*L + l]: only the entries k_slack had to walk agent by agent
    double *node_dsum;                              // [n + N*t] change of the node's injection in this iteration (L > 0)
    double *prev_node;                              // [n + N*t] the node's (this rank's agents') injection sum of the previous iteration (L > 0)
    const double *line_reach;                       // [l] max over nodes of |kap| W_n: beyond it no agent of any node can flip the line's slack
    int *tab_skip;                                  // [t] the price kernel has written the (empty) tables of timestep t
    int *walk_flag, *walk_any;                      // [l + L*t], [t]: the slack sums of (l,t) need the per-node cases (set by the dual step)
    double *part2, *part2_cost;                     // [(n*RB + rb)*T + t], [rb]
    unsigned long long *dual_ticket;                // [1] one-launch dual/price kernel: blocks whose residuals are in (low word) and how many
                                                    // of them saw a residual >= eps (high word)
    // One-launch iterations (one node, no lines, single-GPU chain; kernels_agents.hip "the tail of the iteration inside the
    // x-update launch"): every block of the x-update adds its per-timestep injection sums and its cost into integer
    // accumulators (fixed point + arrival count in one 64-bit atomic add), and one extra block of the launch waits for the
    // counts and runs the whole tail of the iteration. No k_reduce, no dual kernel, one kernel boundary per iteration.
    const TailView *tail;                           // per launch: non-null = this launch chain works that way
    const TailView *tailDev;                        // the context's TailView in device memory (null: not supported for this problem)
    int *reduce_ticket;                             // [n]
    double *cons;
    Status *st;
    const double *node_na;                          // wide chain: [n] agents at node n as a number (k_reduce's naL, read from memory)
};

// The view is every kernel's argument and keeps its layout: a longer DevView moved the register allocation of the fused storage
// kernels. What the extensions add lives BEHIND arrays the view already names — the four blocks below — and
// fmax_ld sits in what was padding in front of gamma.
static_assert(sizeof(DevView) == 832, "DevView must keep its size");
static_assert(offsetof(DevView, fmax_ld) == 172 && offsetof(DevView, gamma) == 176, "fmax_ld fills the padding in front of gamma");

// The storage block (v.sto_emax): S doubles per slot, sorted order, the slots a context holds in this order. The one description of
// the format: dopf_create fills the block from it, the setters take their defaults and destinations from it, and the context's
// host mirror (dopf_ctx::sto_h) has the same shape.
//   emax           the max levels of dopf_create
//   e0             initial levels (DOPF_F_STO_INITIAL_LEVEL: zeros until dopf_set_storage_initial_level)
//   end_lo, end_hi the band of the level after the last timestep (DOPF_F_STO_TERMINAL_LEVEL: [0, emax] until
//                  dopf_set_storage_terminal_level)
//   alpha, beta    al = 1 / eta_d and be = eta_c (DOPF_F_STO_EFFICIENCY: ones until dopf_set_storage_efficiency); the level moves
//                  by be C - al D
enum StoSlot : int { kStoEmax, kStoE0, kStoEndLo, kStoEndHi, kStoAlpha, kStoBeta };
// slots of a context's block, by the plan's level mode (Plan::stoLV): a mode holds every slot below its own, at the defaults
constexpr int kStoSlotsOfLV[4] = {1, 2, 4, 6};
inline int sto_slots(const Plan &p) { return kStoSlotsOfLV[p.stoLV]; }
inline double sto_slot_default(int slot, double emax) { return slot == kStoEmax || slot == kStoEndHi ? emax : slot >= kStoAlpha ? 1.0 : 0.0; }
__host__ __device__ inline const double *sto_slot(const DevView &v, int slot) { return v.sto_emax + (size_t)slot * (size_t)v.S; }
__host__ __device__ inline const double *sto_e0(const DevView &v) { return sto_slot(v, kStoE0); }
__host__ __device__ inline const double *sto_end_lo(const DevView &v) { return sto_slot(v, kStoEndLo); }
__host__ __device__ inline const double *sto_end_hi(const DevView &v) { return sto_slot(v, kStoEndHi); }
__host__ __device__ inline const double *sto_eff_alpha(const DevView &v) { return sto_slot(v, kStoAlpha); }
__host__ __device__ inline const double *sto_eff_beta(const DevView &v) { return sto_slot(v, kStoBeta); }

// The fmax block (v.fmax): one limit per line, or with DOPF_F_LINE_RATING (fmax_ld = L) the L x T rating table — every timestep on
// dopf_create's limits until dopf_set_line_rating — and those L limits behind it (what the central reference reads: it takes no ratings)
inline size_t fmax_doubles(int L, int T, bool rating) { return rating ? (size_t)L * T + (size_t)L : (size_t)L; }
__host__ __device__ inline const double *line_fmax0(const DevView &v) { return v.fmax + (size_t)v.fmax_ld * v.T; }

// The gen_mc block (v.gen_mc): the marginal costs, and with DOPF_F_GEN_QUADRATIC_COST the quadratic coefficients c2[g] behind them,
// sorted order, zeros until dopf_set_generator_quadratic_cost. The cost of row g at output P is gen_mc[g] P + c2[g] P^2 / 2.
inline size_t gen_mc_doubles(int G, bool quad) { return quad ? 2 * (size_t)G : (size_t)G; }
__host__ __device__ inline const double *gen_c2(const DevView &v) { return v.gen_mc + v.G; }

// The gen_pmax block (v.gen_pmax): the generators' capacities, and with DOPF_F_GEN_RAMP behind them, G doubles each in sorted order,
// ramp_up | ramp_down (+inf until dopf_set_generator_ramp) | p_prev (NaN: no anchor), then k_gen_ramp's scratch for the horizons
// whose knots do not fit in LDS (T > kRampLdsT): per wave of the launch (kRampWaves per generator item) kRampRowDoubles(T) doubles —
// T values c_t / y*_t, then the knots' x and v, 2T + 2 each (the bound of DESIGN.md 5r)
constexpr int kRampLdsT = 128, kRampWaves = 8;
__host__ __device__ inline size_t ramp_row_doubles(int T) { return 5 * (size_t)T + 4; }
__host__ __device__ inline size_t ramp_scratch_doubles(int T, int nGenItems) { return T > kRampLdsT ? (size_t)nGenItems * kRampWaves * ramp_row_doubles(T) : 0; }
// ... on a network (DOPF_F_GEN_RAMP_NETWORK, k_gen_ramp_net; L > 0): at every T, per wave p0[T] | y*[T] | kx[K] | kv[K] with
// K = ramp_net_knots(T, L) (ramp_dp.h) — a row's knots leave LDS as soon as the tables' kinks do not fit beside the ramps'
__host__ __device__ inline size_t ramp_scratch_doubles(int T, int nGenItems, int L)
{
    return L > 0 ? (size_t)nGenItems * kRampWaves * ramp_net_row_doubles(T, L) : ramp_scratch_doubles(T, nGenItems);
}
// ... and behind the scratch, where the four arrays and the scratch keep their places, the floors p_min[G] of
// dopf_set_generator_min_output (sorted order, zeros until then): read by the MN instantiations of k_gen_ramp and
// k_gen_ramp_net alone (gen_min_output(v): a ramp context with lines is a DOPF_F_GEN_RAMP_NETWORK one, its scratch the network's)
inline size_t gen_pmax_doubles(int G, int T, int nGenItems, bool ramp, int L = 0)
{
    return ramp ? 5 * (size_t)G + ramp_scratch_doubles(T, nGenItems, L) : (size_t)G;
}
__host__ __device__ inline const double *gen_ramp_up(const DevView &v) { return v.gen_pmax + v.G; }
__host__ __device__ inline const double *gen_ramp_down(const DevView &v) { return v.gen_pmax + 2 * (size_t)v.G; }
__host__ __device__ inline const double *gen_ramp_prev(const DevView &v) { return v.gen_pmax + 3 * (size_t)v.G; }
__host__ __device__ inline double *gen_ramp_scratch(const DevView &v) { return const_cast<double *>(v.gen_pmax) + 4 * (size_t)v.G; }
__host__ __device__ inline const double *gen_min_output(const DevView &v)
{
    return v.gen_pmax + 4 * (size_t)v.G + ramp_scratch_doubles(v.T, v.nGenItems, v.L);
}
// ... with DOPF_F2_GEN_ENERGY_BUDGET (never together with the ramps: plan_chain) behind the capacities, G doubles each in sorted order,
// e_min (0 until dopf_set_generator_energy_budget) | e_max (+inf until then). k_gen_budget keeps nothing else: a searched row forms its
// steps again from P, which it overwrites last (gen_budget.h)
// ... and behind them the rows' budget prices price[G] (sorted order, zeros from dopf_create on): the multiplier the last
// computed x-update put on each budget row, stored by k_gen_budget and read by dopf_get_generator_budget_price alone
inline size_t gen_budget_doubles(int G) { return 4 * (size_t)G; }
__host__ __device__ inline const double *gen_budget_min(const DevView &v) { return v.gen_pmax + v.G; }
__host__ __device__ inline const double *gen_budget_max(const DevView &v) { return v.gen_pmax + 2 * (size_t)v.G; }
// ... with DOPF_F2_GEN_RAMP_BUDGET (both at once, copper plates) the ramps keep their places and the budgets follow them:
// pmax | ramp_up | ramp_down | p_prev | e_min | e_max, then k_gen_ramp_budget's scratch, at every T — per wave of the launch
// (kRampWaves per generator item) the row's centres c[T] and, for each of the 64 candidates a round of the pair search runs, the work
// arrays of the ramp programme, ramp_row_doubles(T), interleaved [slot][lane]
__host__ __device__ inline size_t ramp_budget_wave_doubles(int T) { return (size_t)T + 64 * ramp_row_doubles(T); }
inline size_t gen_ramp_budget_doubles(int G, int T, int nGenItems)
{
    return 7 * (size_t)G + (size_t)nGenItems * kRampWaves * ramp_budget_wave_doubles(T);
}
__host__ __device__ inline const double *gen_rb_min(const DevView &v) { return v.gen_pmax + 4 * (size_t)v.G; }
__host__ __device__ inline const double *gen_rb_max(const DevView &v) { return v.gen_pmax + 5 * (size_t)v.G; }
__host__ __device__ inline double *gen_rb_scratch(const DevView &v) { return const_cast<double *>(v.gen_pmax) + 6 * (size_t)v.G; }
// The budget prices (dopf_get_generator_budget_price), G doubles behind what either layout held before them, so that every other
// offset stays: behind e_max on a DOPF_F2_GEN_ENERGY_BUDGET context, behind the pair search's scratch on a DOPF_F2_GEN_RAMP_BUDGET
// one (as p_min sits behind the ramp scratch). The view does not say which of the two it is: the kernels know (k_gen_ramp_budget:
// pair = true), the host passes Plan::genRampBudget
__host__ __device__ inline double *gen_budget_price(const DevView &v, bool pair)
{
    double *const blk = const_cast<double *>(v.gen_pmax);
    return pair ? blk + 6 * (size_t)v.G + (size_t)v.nGenItems * kRampWaves * ramp_budget_wave_doubles(v.T) : blk + 3 * (size_t)v.G;
}

// The gen_state block (v.gen_state; gen_state_ints). DOPF_F_GEN_AVAILABILITY (the generator bodies' AV instantiations): cap[g,t] = gen_pmax[g] * f[t + T*k] with k = gen_prof(v)[g],
// gen_pmax[g] for k = -1. gen_state has room for both behind its G row states: the G profile indices (sorted order, -1 until
// dopf_set_generator_availability), then, on the next 8-byte boundary, the device address of the profile table f (grown by the
// setter). The view, every kernel's argument, keeps its layout: a longer DevView moved the register allocation of the fused
// storage kernels.
__host__ __device__ inline int *gen_prof(const DevView &v) { return v.gen_state + v.G; }
__host__ __device__ inline const double **gen_avail_slot(const DevView &v)
{
    return reinterpret_cast<const double **>(v.gen_state + ((2 * (size_t)v.G + 1) & ~(size_t)1));
}
inline size_t gen_state_ints(int G, bool avail) { return avail ? ((2 * (size_t)G + 1) & ~(size_t)1) + 2 : (size_t)G; }

// DOPF_F_GEN_AVAILABILITY (the AV instantiations of the generator bodies, kernels_agents.hip and kernels_central.hip): the row's upper bound at a timestep, cap = pmax * f with f
// the row's profile value — one fp64 multiply, never contracted into the sums that add it (a kept row adds cap itself, and the full
// sweep adds the clamped value: both must be the same bits). prof < 0: pmax, no shape is read.
__device__ __forceinline__ double avail_mul(double pm, double f)
{
#pragma clang fp contract(off)
    return pm * f;
}

// (f: the profile table, *gen_avail_slot(v), loaded once per block)
__device__ __forceinline__ double avail_cap(const double *f, int T, int prof, double pm, int t)
{
    return prof >= 0 ? avail_mul(pm, f[(size_t)prof * T + t]) : pm;
}

// check_convergence!, convergence.jl:1-31 (one thread). The status words a stop test starts from are loaded early by
// callers that can (a load at the very end of a one-block kernel is a round trip on its critical path).
struct StatusPre { int iteration, converged, iters_total; };
__device__ __forceinline__ StatusPre status_load(const DevView &v)
{
    StatusPre s;
    s.iteration = v.st->iteration; s.converged = v.st->converged; s.iters_total = v.st->iters_total;
    return s;
}

__device__ __forceinline__ void status_update(const DevView &v, const StatusPre s, double r0, double r1, double r2)
{
    Status *st = v.st;
    int conv = s.converged, it = s.iteration;
    if (it != 1) {                                                        // convergence.jl:3
        st->res[0] = r0; st->res[1] = r1; st->res[2] = r2;
        st->res_set = -1;
        conv = (r0 < v.eps) && (r1 < v.eps) && (r2 < v.eps);
        st->converged = conv;
    }
    st->iters_total = s.iters_total + 1;
    if (!conv) it += 1;                                                   // convergence.jl:25-30
    st->iteration = it;
    st->halt = conv || (v.max_iters > 0 && it > v.max_iters);
}

__device__ __forceinline__ void status_update(const DevView &v, double r0, double r1, double r2)
{
    status_update(v, status_load(v), r0, r1, r2);
}

// f(LPS, NCH) for the plan's lane group, as std::integral_constant arguments, over the first NP pairs of kStoPairs only: a launch
// family is instantiated for exactly those. plan_chain refuses a lane group that the families it chose do not cover.
template <int NP, int I = 0, class F>
void with_sto_pair(const Plan &p, F &&f)
{
    if constexpr (I < NP) {
        if (p.stoLPS == kStoPairs[I][0] && p.stoNCH == kStoPairs[I][1])
            f(std::integral_constant<int, kStoPairs[I][0]>{}, std::integral_constant<int, kStoPairs[I][1]>{});
        else
            with_sto_pair<NP, I + 1>(p, f);
    }
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument (both are instantiated)
template <class F>
void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(integral_constant<int, LV>) for the plan's level mode p.stoLV (0 .. 3: all four instantiated)
template <class F>
void with_lv(int lv, F &&f)
{
    if (lv == 3) f(std::integral_constant<int, 3>{});
    else if (lv == 2) f(std::integral_constant<int, 2>{});
    else if (lv == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// the central reference's view (kernels_central.hip): the context's arrays (P, D, C, E, items, partial sums, cons) plus the
// multipliers, running sums and step sizes of the primal-dual iteration
struct CentralView {
    DevView v;
    double *yb, *yf, *yE;                   // multipliers: balance [T], flows [l + L*t], levels [t + T*s]
    double *aP, *aD, *aC, *aE, *ab, *af;    // running sums of the iterates since the last restart
    double *pi;                             // [n + N*t] yb + ptdf' yf of the candidate being worked on
    const double *tauN;                     // [n] 1 / (1 + sum_l |ptdf[l,n]|): primal step of a generator at node n
    const double *absHn;                    // [n] sum_l |ptdf[l,n]|
    const double *sigF;                     // [l] 1 / sum_n |ptdf[l,n]| (units at n, a storage counting twice)
    double sigB, w;                         // 1 / (G + 2S); primal weight
    double *m_gen, *m_sto, *m_dual;         // metrics: per generator item [1], per storage item [3], per timestep [3]
    // dopf_central_solve_coupled (central_rows.h). rows_in non-null: kc_gen_rows runs in kc_gen's place; rated: kc_dual<., true>
    const double *rows_in;                  // [5][G], sorted order: ramp_up | ramp_down | p_prev (NaN: no anchor) | e_min | e_max
    double *yR, *yQ;                        // multipliers: ramp rows [t + T*g] (t = 0: the anchor's row), budget rows [g]
    double *aR, *aQ;                        // ... their running sums since the last restart
    double *m_rows;                         // metrics: per generator item [3] reduced-cost term, rows' support term, worst row violation
    int rated;                              // the flow rows' limits are the rating table v.fmax[l + L*t], not line_fmax0(v)[l]
    int longRows;                           // kc_gen_rows_long in kc_gen_rows' place: T > 512, or DOPF_F_DEBUG_LONG_STO (read with rows_in)
};

// the horizon kc_sto and kc_gen_rows hold in one wave's registers (64 lanes x 8 timesteps, the one-wave storage bodies' limit:
// sto_config_supported); beyond it kc_sto_long and kc_gen_rows_long run
constexpr int kCentralWaveHorizon = 64 * 8;

// kernels_central.hip
// (p: the context's plan — genAvail and stoLV select the sweeps' feature instantiations)
void central_launch_iteration(const CentralView &c, const Plan &p, const DevView &vreduce, hipStream_t s);
// (XR, XQ: the candidate's ramp and budget multipliers; read only with c.rows_in)
void central_launch_metrics(const CentralView &c, const Plan &p, const DevView &vreduce, const double *XP, const double *XD, const double *XC,
                            const double *XE, const double *yb, const double *yf, const double *XR, const double *XQ, double scale, hipStream_t s);
void central_launch_scale_copy(double *dst, const double *src, double scale, size_t n, hipStream_t s);
constexpr int kCentralDiffBlocks = 256;
int central_diff_blocks(size_t n);           // blocks (= partial sums) central_launch_diff_sq writes for n values, at most kCentralDiffBlocks
void central_launch_diff_sq(const double *a, const double *b, size_t n, double *part, hipStream_t s);   // part[block] = sum (a - b)^2
void central_launch_scale_copy_primal(const CentralView &c, const Plan &p, double scale, hipStream_t s);   // P, D, C from their running sums, inside the boxes

// Blocks of an x-update that add their sums to the one-launch tail: the storage items and the generator items — or, in the fused
// launch's streaming form (genBlocks > 0 only there), its generator blocks. The fused launch's grid (+ the tail block) and
// TailView::expect are this one count.
inline int agent_blocks(const DevView &v) { return v.nStoItems + (v.genBlocks > 0 && !v.genSkip ? v.genBlocks : v.nGenItems); }

// kernels_agents.hip
void launch_gen_update(const DevView &v, const Plan &p, hipStream_t s);
void launch_gen_ramp(const DevView &v, const Plan &p, hipStream_t s);       // gen_ramp.h: the generators of a DOPF_F_GEN_RAMP context
void launch_gen_ramp_net(const DevView &v, const Plan &p, hipStream_t s);   // gen_ramp_net.h: ... on a network (DOPF_F_GEN_RAMP_NETWORK)
void launch_gen_budget(const DevView &v, const Plan &p, hipStream_t s);     // gen_budget.h: the generators of a DOPF_F2_GEN_ENERGY_BUDGET context
void launch_gen_budget_win(const DevView &v, const Plan &p, hipStream_t s); // gen_budget_win.h: ... while dopf_set_generator_energy_budget_windows holds a table
void launch_gen_ramp_budget(const DevView &v, const Plan &p, hipStream_t s);   // gen_ramp_budget.h: ... of a DOPF_F2_GEN_RAMP_BUDGET context
void launch_sto_update(const DevView &v, const Plan &p, hipStream_t s);
void launch_net_agents(const DevView &v, const Plan &p, hipStream_t s);
void launch_agents_fused(const DevView &v, const Plan &p, hipStream_t s);
int debug_timeline(unsigned long long *out, int n);     // DOPF_STATS builds: per-wave stamps of the storage body
// kernels_consensus.hip
hipError_t raise_lds_limits(const DevView &v, const Plan &p);        // dopf_create, on the context's device: the dynamic LDS the plan's kernels need
void launch_tables(const DevView &v, const Plan &p, hipStream_t s);
void launch_slack(const DevView &v, hipStream_t s);
void launch_reduce(const DevView &v, const Plan &p, hipStream_t s);
// Peer exchange (dopf_comm.hip sets it up): every rank owns a receive area [2 parities][world source ranks][n doubles] plus
// flags [2][world][chunks]; data[r] / flags[r] are rank r's areas as addressable from THIS device (own allocation, a peer
// device of the same process, or an IPC mapping of another process's allocation).
constexpr int kXchgMaxWorld = 16;
constexpr int kXchgChunk = 2048;                // doubles per block
struct XchgView {
    int world, me, nchunks;
    int rs;                                     // 1: reduce-scatter + all-gather form (k_xchg_rs: vectors of more than one chunk per rank)
    unsigned long long n;                       // doubles in the consensus vector
    unsigned long long timeout_ticks;           // wall_clock64 ticks (100 MHz) a block waits for its peers
    double *data[kXchgMaxWorld];
    unsigned long long *flags[kXchgMaxWorld];
    double *sum[kXchgMaxWorld];                 // [2 parities][n]: the summed chunks, written by each chunk's owner (rs form)
    unsigned long long *sflags[kXchgMaxWorld];  // [2][chunks]
};
void launch_xchg(const DevView &v, const XchgView &x, hipStream_t s, bool inj_only = false);   // cons <- sum over ranks of cons (rank order);
//      // inj_only: just the chunks that hold the node sums and the cost (the slack sums are formed behind the exchange: slackGlobal)
void launch_dual(const DevView &v, const Plan &p, hipStream_t s, const XchgView *xd = nullptr);   // xd: peer exchange inside the one-block kernel
//      // consensus -> duals, residuals, prices, status
void launch_derive(const DevView &v, const Plan &p, hipStream_t s, bool from_primal);
void launch_derive_level(const DevView &v, const Plan &p, hipStream_t s);   // E = e0 + cumsum(C - D) into v.E (e0 = 0 without p.stoE0; p.stoEff: be C - al D)
// dopf_set_demand / dopf_roll_horizon (kernels_consensus.hip). A per-timestep vector [j + stride*t] that moves by k
// timesteps through the scratch (at off); tail: what follows the kept part (stride*k values), null: the old last timestep
struct RollVec { double *p; const double *tail; size_t off; int stride; };
struct RollVecs { RollVec a[12]; double *scratch; int n; };
void launch_roll_level(const DevView &v, const Plan &p, int k, bool from_E, double *out /* S, device */, hipStream_t s);   // clamped level after timestep k - 1
// dopf_roll_horizon_coupled, before the rows move: out = P[:, k-1] | e_min' | e_max' | spent, G doubles each, sorted
// order; e_min / e_max: the stored bounds on the device, or both null (the anchor alone is written)
void launch_roll_gen_window(const DevView &v, int k, const double *e_min, const double *e_max, double *out /* 4G, device */, hipStream_t s);
void launch_roll_vecs(const RollVecs &rv, int T, int k, hipStream_t s);
// P, D, C moved by k in place (k = 0: left alone), the node sums formed from the rows item by item, status (iteration <= 0: kept)
// and the derived consensus state as dopf_set_state leaves them
void launch_roll_state(const DevView &v, const Plan &p, int k, int iteration, hipStream_t s);
// dopf_set_line_rating: status as dopf_set_demand leaves it, then the consensus step's derived state under the new limits — the
// per-(l,t) flags, walk_any / tab_skip and the tables the price kernels write — from the sums in cons (no sums are formed or moved)
void launch_line_rating(const DevView &v, const Plan &p, hipStream_t s);
// dopf_set_generator_quadratic_cost, dopf_set_generator_ramp, dopf_set_generator_min_output: status as dopf_set_line_rating leaves it (nothing derived depends on the costs or the ramps)
void launch_reset_status(const DevView &v, hipStream_t s);
void launch_penalty_sums(const DevView &v, double *out /* [3][N][T], device */, hipStream_t s);   // Result.penalty_term, per node
void launch_node_results(const DevView &v, double *gen, double *dis, double *chg, hipStream_t s);   // [n + N*t] each, device pointers   // consensus -> inj/s/flow/price (no dual step)

}  // namespace dopf
