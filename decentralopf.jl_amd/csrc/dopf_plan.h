// dopf_plan.h — what dopf_create decides before it touches the device, as plain C++ (no HIP include: tests/test_plan_chain.py
// compiles this header alone, with sanitizers, and pins its output):
//   plan_chain   which kernels a context runs, from the problem's shape, the flags and the CU count
//   make_layout  where the agents' work lands: the work items, their rows in the transposed partial sums, the reduce blocks and the
//                one-launch dual kernel's LDS map — the only code that cuts items or counts rows (plan_chain takes its counts from it)
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/dopf.h"
#include "budget_win_map.h"

namespace dopf {

// Sizing knobs of the experiments (item and block counts, the exchange's rendezvous wait) are environment
// variables of builds with -DDOPF_EXPERIMENTS only; none of them chooses a kernel. plan_chain reads them (and the exchange its own).
#ifdef DOPF_EXPERIMENTS
inline const char *exp_env(const char *name) { return getenv(name); }
#else
inline const char *exp_env(const char *) { return nullptr; }
#endif

// one block's share of the agent list: agents [a0, a1) all sit at `node`
struct Item {
    int a0, a1, node, row;          // row (networks): the item's row in DevView::part_T (a storage item's scan partial; its warm-start partial: row + 1)
};

#ifndef DOPF_ACC_REP
#define DOPF_ACC_REP 16
#endif
constexpr int kAccRep = DOPF_ACC_REP;     // replicas of the accumulators (a block adds into replica blockIdx % kAccRep: 1/16 of the adds per address)

// consensus states up to this many (n,t) / (l,t) entries take the one-block dual step
constexpr size_t kSmallConsensus = 4096;
#ifndef DOPF_STREAM_ROWS
#define DOPF_STREAM_ROWS 6
#endif
constexpr int kGenStreamRows = DOPF_STREAM_ROWS;          // rows per lane and item in the streaming generator blocks (one batch of loads)

// The consensus step (dual update, prices, stop test): k_dual_price_small (state <= kSmallConsensus entries), k_dual_price_t1024
// (networks, N and L <= 256), k_dual_t + k_price_t (a timestep's vectors in 48 KB of LDS), k_dual + k_price, the wide chain (net_wide.h)
enum class Consensus : int { Small, T1024, DualT, Generic, Wide };

// The launch chain of a context: every create-time choice of which kernels run, made once by plan_chain.
// Kernels read the parts they need from DevView; the rest is read by the host's launch functions only.
struct Plan {
    const char *refusal;            // non-null: no kernel instantiation serves this problem (DOPF_E_UNSUPPORTED)
    int stoLPS, stoNCH;             // storage lane group: lanes per storage x timesteps per lane (sto_config_supported)
    int stoLong;                    // the long-horizon storage body (sto_long.h: DOPF_F_LONG_HORIZON beyond T = 512, DOPF_F_DEBUG_LONG_STO)
    int wideNet;                    // the wide chain (net_wide.h: DOPF_F_WIDE_NETWORK beyond L = 2048, DOPF_F_DEBUG_WIDE_NET): no one-launch,
                                    // quiet or tail chain
    Consensus consensus;
    bool sliceDual;                 // the one-block dual kernel may add k_reduce's slices itself (DevView::sliceDual)
    bool useWarm, stoLean;          // storage warm start (DevView::use_warm); the lean active-set body (sto_lean.h)
    bool genAvail;                  // DOPF_F_GEN_AVAILABILITY: the generator bodies that read the rows' profiles (nothing else of the plan changes)
    bool genQuad;                   // DOPF_F_GEN_QUADRATIC_COST: the generators run in k_gen_update<.., .., QC> on every shape — no pair, skip or fused
                                    // generator blocks, no one-launch tail (the chain of DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE at odd T)
    bool genRamp;                   // DOPF_F_GEN_RAMP (copper plates): the generators run in k_gen_ramp<AV, QC> — the chain of genQuad (no pair, skip or
                                    // fused generator blocks, no one-launch tail), with the exact projection onto {box, ramps} for the rows that need it
    bool genRampNet;                // ... on a network (DOPF_F_GEN_RAMP_NETWORK, L > 0): k_gen_ramp_net<AV, QC>, the chain a network runs under DOPF_F_NO_FUSE
    bool genBudget;                 // DOPF_F2_GEN_ENERGY_BUDGET (the second flag word): k_gen_budget<LINES, AV, QC> (gen_budget.h) on the same chain, copper
                                    // plates and networks; refused together with genRamp unless ...
    bool genRampBudget;             // DOPF_F2_GEN_RAMP_BUDGET (copper plates, with genRamp and genBudget): k_gen_ramp_budget<AV, QC> (gen_ramp_budget.h)
                                    // on the same chain — the ramp programme inside the budget's multiplier search
    bool genMinOut;                 // the MN instantiations of k_gen_ramp / k_gen_ramp_net. The one entry plan_chain never sets: no
                                    // flag asks for it — dopf_set_generator_min_output switches it on a genRamp context (and drops the graphs)
    bool genBudgetPrice;            // the PR instantiations of k_gen_budget, which store the rows' budget prices. Like genMinOut never set by
                                    // plan_chain: the first dopf_get_generator_budget_price switches it on a genBudget context (and drops the graphs)
    double *genRampPrice;           // non-null: the RP instantiations of k_gen_ramp / k_gen_ramp_budget store the rows' ramp multipliers
                                    // there (T x G doubles of the context's own, the kernels' second argument). Like genMinOut never set by plan_chain:
                                    // the first dopf_get_generator_ramp_price allocates it on a copper-plate genRamp context (and drops the graphs)
    BudgetWinView genBudgetWin;     // n_win > 0: k_gen_budget_win<LINES, AV, QC> (gen_budget_win.h) runs for k_gen_budget, with this as its second
                                    // argument: the window ends, budgets and prices of the context's own. Like genMinOut never set by plan_chain:
                                    // dopf_set_generator_energy_budget_windows sets and clears it on a genBudget context (and drops the graphs)
    double *genBudgetMinOut;        // non-null: the MN instantiations of k_gen_budget / k_gen_budget_win read the rows' floors there (G
                                    // doubles of the context's own, sorted order; the kernels' last argument). Like genMinOut never set by plan_chain:
                                    // dopf_set_generator_budget_min_output sets it with an array and clears it with NULL (and drops the graphs)
    bool stoE0;                     // DOPF_F_STO_INITIAL_LEVEL: initial levels in sto_e0(v) (k_derive_level reads them)
    int stoLV;                      // the storage bodies' level mode: 0 none, 1 initial levels (DOPF_F_STO_INITIAL_LEVEL), 2 initial levels
                                    // and terminal bands (DOPF_F_STO_TERMINAL_LEVEL; sto_e0(v) holds zeros without the first flag), 3 those
                                    // and efficiencies (DOPF_F_STO_EFFICIENCY; defaults for what the other two flags do not set)
    bool stoEff;                    // DOPF_F_STO_EFFICIENCY: levels are e0 + cumsum(be C - al D) (k_derive_level_eff, k_roll_level_eff)
    bool fuseAgents, fuseNet;       // generators + storages in one launch: k_agents (copper plate, even T), k_net_agents (networks)
    bool tail;                      // the tail of the iteration in the x-update launch (DevView::tailDev)
    bool slackDual;                 // the one-launch dual/price kernel may form the slack sums: no k_reduce (DevView::slackInDual)
    bool quiet, commQuiet;          // the quiet chain may run: single GPU (DevView::quiet), on a peer exchange (DevView::slackGlobal)
    int genTT, genR, genTT2, genR2, genTT256, genSkip, genBlocks, tablesInDual;     // (DevView)
    int genItem, stoItem;           // agents per generator / storage work item
    int nGenItems, nStoItems, rowsT;
};

// (lanes per storage, timesteps per lane) of the one-wave storage bodies. A launch family is instantiated for a prefix of the list:
// k_agents / k_net_agents for kFusedPairs, the storage launches for all.
constexpr int kStoPairs[][2] = {{8, 1}, {8, 2}, {8, 3}, {16, 3}, {32, 3}, {64, 3}, {64, 6}, {64, 8}};
constexpr int kFusedPairs = 6, kAllPairs = 8;

// the lane group of the one-wave storage bodies at horizon T (false: none, the long body's horizons)
inline bool sto_config_supported(int T, Plan *p)
{
    // lane group x consecutive timesteps per lane; 3 timesteps per lane keeps the kernel at 2 waves/SIMD
    if (T <= 24) { p->stoLPS = 8; p->stoNCH = (T + 7) / 8; return true; }
    if (T <= 48) { p->stoLPS = 16; p->stoNCH = 3; return true; }
    if (T <= 96) { p->stoLPS = 32; p->stoNCH = 3; return true; }
    if (T <= 192) { p->stoLPS = 64; p->stoNCH = 3; return true; }
    if (T <= 384) { p->stoLPS = 64; p->stoNCH = 6; return true; }
    if (T <= 512) { p->stoLPS = 64; p->stoNCH = 8; return true; }
    return false;
}

// the wide chain (net_wide.h): beyond 2048 lines, where k_tables' LDS (4 * 2L doubles) runs out, or at any L on request
inline bool wide_chain(int L, unsigned flags) { return 2 * L > 4096 || (L > 0 && (flags & DOPF_F_DEBUG_WIDE_NET)); }

// the quiet chain's dual/price kernel stages every partial row of its timestep in LDS: up to 96 KB of them
inline bool quiet_rows_fit(int rows) { return rows > 0 && (size_t)rows * sizeof(double) <= 96 * 1024; }

// The problem's sizes and what plan_chain needs of its data
struct Shape {
    int N, L, T, G, S;
    std::vector<int> gen_at, sto_at;    // generators / storages per node (the node-sorted agent lists, counted)
    int ki, kc;                         // fraction bits the fixed-point sums of the one-launch tail would keep (injection, cost)
};

// What make_layout returns: the work items (row: a POSITION, see DevView::part_T), the agent and item ranges per node (N + 1 each),
// the rows' placement and the scalars of DevView with the same names
struct Layout {
    std::vector<Item> gen_items, sto_items;
    std::vector<int> node_gen_beg, node_sto_beg, node_gitem_beg, node_sitem_beg;
    std::vector<int> row_of_pos, pos_of_row;        // networks only (empty on a copper plate)
    int rowsN = 0, rowsT = 0;
    int maxNodeAgents = 0, reduceRB = 1;
    int dualRowsOff = 0, dualSdOff = 0, dualLdsBytes = 0;
};

// split the node-sorted agent list (per_node: agents at each node) into block work items that never cross a node boundary
inline void make_items(const std::vector<int> &per_node, int chunk, std::vector<Item> &items, std::vector<int> &node_beg,
                       std::vector<int> &node_item_beg)
{
    const int N = (int)per_node.size();
    node_beg.assign(N + 1, 0);
    for (int n = 0; n < N; ++n) node_beg[n + 1] = node_beg[n] + per_node[n];
    node_item_beg.assign(N + 1, 0);
    items.clear();
    for (int n = 0; n < N; ++n) {
        node_item_beg[n] = (int)items.size();
        for (int a = node_beg[n]; a < node_beg[n + 1]; a += chunk)
            items.push_back(Item{a, std::min(a + chunk, node_beg[n + 1]), n, 0});
    }
    node_item_beg[N] = (int)items.size();
}

// The items of both agent kinds and, on a network, their rows in the transposed partial sums (DevView::part_T): node n owns rows
// [g0 + 2 s0, ...) — its generator items, then two per storage item (node order: generator item i -> i + 2 s0, storage item
// k -> g0' + 2 k and the row behind it). The rows are then placed by the XCD (of eight) whose blocks write them — storage item k:
// k % 8, generator item i: i % 8 behind the storage blocks of the fused launch (k_net_agents: storages first) — each XCD's rows
// padded to 16. Fills everything of lo but the reduce blocks and the LDS map.
inline void place_items(const Shape &sh, int genItem, int stoItem, bool fuseNet, Layout &lo)
{
    make_items(sh.gen_at, genItem, lo.gen_items, lo.node_gen_beg, lo.node_gitem_beg);
    make_items(sh.sto_at, stoItem, lo.sto_items, lo.node_sto_beg, lo.node_sitem_beg);
    for (int n = 0; n < sh.N; ++n) lo.maxNodeAgents = std::max(lo.maxNodeAgents, sh.gen_at[n] + sh.sto_at[n]);
    if (sh.L == 0) return;
    const int nG = (int)lo.gen_items.size(), nS = (int)lo.sto_items.size();
    lo.rowsN = nG + 2 * nS;
    std::vector<int> xcd((size_t)lo.rowsN, 0), cnt(8, 0), beg(9, 0);
    for (int i = 0; i < nG; ++i) {
        lo.gen_items[i].row = i + 2 * lo.node_sitem_beg[lo.gen_items[i].node];
        xcd[(size_t)lo.gen_items[i].row] = ((fuseNet ? nS : 0) + i) % 8;
    }
    for (int k = 0; k < nS; ++k) {
        lo.sto_items[k].row = lo.node_gitem_beg[lo.sto_items[k].node + 1] + 2 * k;
        xcd[(size_t)lo.sto_items[k].row] = xcd[(size_t)lo.sto_items[k].row + 1] = k % 8;
    }
    for (int g = 0; g < lo.rowsN; ++g) ++cnt[(size_t)xcd[(size_t)g]];
    for (int x = 0; x < 8; ++x) beg[(size_t)x + 1] = beg[(size_t)x] + (cnt[(size_t)x] + 15) / 16 * 16;
    lo.rowsT = beg[8];
    lo.row_of_pos.assign((size_t)std::max(lo.rowsT, 1), -1);
    lo.pos_of_row.assign((size_t)std::max(lo.rowsN, 1), 0);
    for (int g = 0; g < lo.rowsN; ++g) {
        const int at = beg[(size_t)xcd[(size_t)g]]++;
        lo.row_of_pos[(size_t)at] = g;
        lo.pos_of_row[(size_t)g] = at;
    }
    for (Item &it : lo.gen_items) it.row = lo.pos_of_row[(size_t)it.row];
    for (Item &it : lo.sto_items) it.row = lo.pos_of_row[(size_t)it.row];       // (the warm-start row: the next position)
}

// The launch chain of a context, decided once: make_layout builds the items and rows from it, the launch functions
// switch on it. No HIP call, no device allocation. cus: the device's CUs (0: unknown). dopf_create has refused T > 512 without
// DOPF_F_LONG_HORIZON and L > 2048 without DOPF_F_WIDE_NETWORK. flags2: the second flag word (DOPF_F2_*, dopf_create_ex).
inline Plan plan_chain(const Shape &sh, unsigned flags, int cus, unsigned flags2 = 0)
{
    const int N = sh.N, L = sh.L, T = sh.T, G = sh.G, S = sh.S;
    Plan p{};
    if (S > 0 && (!sto_config_supported(T, &p) || (flags & DOPF_F_DEBUG_LONG_STO))) p.stoLong = 1;
    if (p.stoLong) { p.stoLPS = 64; p.stoNCH = 8; }         // (not read by the long body; keeps the one-wave paths' choices off)
    p.wideNet = wide_chain(L, flags) ? 1 : 0;
    p.useWarm = S > 0 && p.stoNCH <= 3 && !(flags & DOPF_F_NO_WARM_START);     // (the long body: NCH 8, off)
    // The lean active-set body (sto_lean.h): 32-bit element offsets; on a network only where the storage blocks outnumber the
    // chip's resident slots several times — its gain is instruction count, and a grid of one resident round is bound by one
    // block's latency chain, which is no shorter (configs[3]: 114 us against 120 at 100 k agents; its 12.5 k share 43.3 against 41.1).
    // DOPF_F_STO_INITIAL_LEVEL / DOPF_F_STO_TERMINAL_LEVEL: the general bodies' level-mode instantiations (a level before timestep 0;
    // and a band after the last one); the lean body has none
    p.stoE0 = S > 0 && (flags & DOPF_F_STO_INITIAL_LEVEL);
    // DOPF_F_GEN_AVAILABILITY: the same chain, with the generator bodies' AV instantiations (cap <= gen_pmax: every bound derived
    // from gen_pmax below and in dopf_create stays valid)
    p.genAvail = G > 0 && (flags & DOPF_F_GEN_AVAILABILITY);
    // DOPF_F_STO_EFFICIENCY: level mode 3 whatever the other two flags say (e0 and the band at their defaults without them) — one more
    // instantiation per storage launch family; the chain is the one the same problem runs with the other two flags
    p.stoEff = S > 0 && (flags & DOPF_F_STO_EFFICIENCY);
    p.stoLV = S == 0 ? 0 : p.stoEff ? 3 : (flags & DOPF_F_STO_TERMINAL_LEVEL) ? 2 : (flags & DOPF_F_STO_INITIAL_LEVEL) ? 1 : 0;
    p.stoLean = !((flags & (DOPF_F_STO_GENERAL | DOPF_F_STO_INITIAL_LEVEL | DOPF_F_STO_TERMINAL_LEVEL | DOPF_F_STO_EFFICIENCY)) ||
                  (unsigned long long)S * T * sizeof(double) >= (1ull << 32) ||
                  (L > 0 && (long long)S * p.stoLPS / 256 < 1024)) && !p.stoLong;
    p.genTT = std::min(T, 512);
    p.genR = 512 / p.genTT;
    // DOPF_F_GEN_QUADRATIC_COST: the generators in k_gen_update's QC instantiations, a launch of their own on every shape — no pair
    // or skip kernels (genTT2 = 0, and with it no one-launch tail: `pairs` below), no k_agents, no k_net_agents. The chain the
    // same problem runs under DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE at odd T; the storages' launch of that chain, with the LV above
    p.genQuad = G > 0 && (flags & DOPF_F_GEN_QUADRATIC_COST);
    // DOPF_F_GEN_RAMP: the same chain with k_gen_ramp as the generators' launch on a copper plate; on a network the row's derivative
    // gains up to 2L kinks per step — k_gen_ramp_net, behind DOPF_F_GEN_RAMP_NETWORK (its knot scratch grows with the tables: the
    // caller asks for it). That flag alone is refused; with L == 0 it is ignored
    p.genRamp = G > 0 && (flags & DOPF_F_GEN_RAMP);
    p.genRampNet = p.genRamp && L > 0 && (flags & DOPF_F_GEN_RAMP_NETWORK);
    if ((flags & DOPF_F_GEN_RAMP) && L > 0 && !(flags & DOPF_F_GEN_RAMP_NETWORK))
        p.refusal = "ramp limits run on copper plates; on a network they need DOPF_F_GEN_RAMP_NETWORK at dopf_create";
    if ((flags & DOPF_F_GEN_RAMP_NETWORK) && !(flags & DOPF_F_GEN_RAMP))
        p.refusal = "DOPF_F_GEN_RAMP_NETWORK means nothing without DOPF_F_GEN_RAMP";
    // DOPF_F2_GEN_ENERGY_BUDGET: the same chain again with k_gen_budget as the generators' launch, on every shape. With ramps a row
    // would carry two constraints that couple its timesteps (the ramp programme inside the multiplier search): refused
    p.genBudget = G > 0 && (flags2 & DOPF_F2_GEN_ENERGY_BUDGET);
    if ((flags2 & DOPF_F2_GEN_ENERGY_BUDGET) && (flags & DOPF_F_GEN_RAMP) && !(flags2 & DOPF_F2_GEN_RAMP_BUDGET))
        p.refusal = "DOPF_F2_GEN_ENERGY_BUDGET does not combine with DOPF_F_GEN_RAMP: one constraint that couples a generator's timesteps per context";
    // DOPF_F2_GEN_RAMP_BUDGET: the pair on a copper plate, the same chain with k_gen_ramp_budget as the generators' launch (the ramp
    // programme inside the multiplier search; its scratch grows with T: the caller asks for it). Alone it is refused, as on a network
    p.genRampBudget = G > 0 && L == 0 && (flags2 & DOPF_F2_GEN_RAMP_BUDGET) && (flags2 & DOPF_F2_GEN_ENERGY_BUDGET) && (flags & DOPF_F_GEN_RAMP);
    if (flags2 & DOPF_F2_GEN_RAMP_BUDGET) {
        if (!((flags2 & DOPF_F2_GEN_ENERGY_BUDGET) && (flags & DOPF_F_GEN_RAMP)))
            p.refusal = "DOPF_F2_GEN_RAMP_BUDGET means nothing without DOPF_F_GEN_RAMP and DOPF_F2_GEN_ENERGY_BUDGET";
        else if (L > 0)
            p.refusal = "DOPF_F2_GEN_RAMP_BUDGET runs on copper plates: DOPF_F_GEN_RAMP and DOPF_F2_GEN_ENERGY_BUDGET do not combine on a network";
    }
    if (p.genQuad || p.genRamp || p.genBudget) flags |= DOPF_F_NO_FUSE;
    p.genTT2 = (!p.genQuad && !p.genRamp && !p.genBudget && L == 0 && T % 2 == 0 && T / 2 <= 512) ? T / 2 : 0;
    p.fuseAgents = p.genTT2 > 0 && p.genTT2 <= 256 && G > 0 && S > 0 && p.useWarm && !(flags & (DOPF_F_NO_FUSE | DOPF_F_OVERLAP_AGENTS));
    if (p.fuseAgents) {
        // one launch for all agents pays while its fixed cost matters and every storage block is resident from
        // the start (3 blocks of 256 per CU at the storage code's register count); see k_agents
        const int ng = 256 / p.stoLPS;
        const int sch = (std::max(ng, (S + 2047) / 2048) + ng - 1) / ng * ng;
        const long long sto_blocks = (S + sch - 1) / sch + N - 1;
        if (sto_blocks > 3 * 256 || (long long)G * T > (8ll << 20)) p.fuseAgents = false;
    }
    p.genR2 = p.genTT2 ? (p.fuseAgents ? 256 : 512) / p.genTT2 : 0;
    // networks: generators and storages in one launch (k_net_agents) unless the storages run on a stream of their own
    p.genTT256 = std::max(1, std::min((std::min(T, 512) + 1) / 2, 256 / p.genR));
    p.fuseNet = L > 0 && G > 0 && S > 0 && p.useWarm && !(flags & (DOPF_F_NO_FUSE | DOPF_F_OVERLAP_AGENTS)) &&
                p.genR * p.genTT256 <= 256;          // (T = 1: the 512-thread tiling has more agent lanes than such a block has threads)
    // One-launch iterations (kernels_agents.hip, "the tail of the iteration inside the x-update launch"): the fixed-point sums need
    // 8 fraction bits of the injection and a non-negative exponent of the cost (64 bits = sign + 53 value bits + the 10-bit arrival count)
    const bool pairs = p.genTT2 > 0 && (S == 0 || p.useWarm) && G + S > 0;       // pair kernels / k_agents / k_sto
    p.tail = N == 1 && L == 0 && pairs && sh.ki >= 8 && sh.kc >= 0 &&
             !(flags & (DOPF_F_NO_TAIL_FUSE | DOPF_F_OVERLAP_AGENTS));          // (two streams: the storage launch does not follow the generators')

    // work items
    const int R = p.genTT2 ? p.genR2 : p.genR;
    // ~2048 blocks fill the chip several times over; in the fused launch the generator blocks share the wave slots with
    // the storage blocks and ~1536 somewhat larger ones come out ahead (measured on config2: 25.7 -> 24.0 us)
    // (with lines ~1024 blocks: the 118-node share 93.8 -> 87.3 us per iteration, config3 at full size 204 -> 203)
    // (networks, one launch for all agents: the generator blocks pass through the ~230 wave slots the storage blocks leave
    // free at that kernel's register count — ~512 larger ones: the 118-node share 51.6 -> 49.5 us per iteration)
    int target_items = p.fuseAgents ? 1536 : (L > 0 ? ((p.fuseNet && !(flags & DOPF_F_NET_SMALL_ITEMS)) ? 512 : 1024) : 2048);
    if (const char *e = exp_env("DOPF_GEN_TARGET_ITEMS")) target_items = std::max(1, atoi(e));     // (experiments)
    // streaming generator blocks (fused launch, one node): an item is ONE batch of loads, <= kGenStreamRows rows per lane
    const bool stream = p.fuseAgents && N == 1;
    if (stream) target_items = std::max(target_items, (G + kGenStreamRows * R - 1) / (kGenStreamRows * R));
    int chunk = std::max(R, (G + target_items - 1) / target_items);
    chunk = (chunk + R - 1) / R * R;
    if (stream) chunk = std::min(chunk, kGenStreamRows * R);
    p.genItem = chunk;
    // (on short blocks the skip test costs more than the rows it saves: measured on config1/config2)
    p.genSkip = (p.genTT2 > 0 && chunk >= 8 * R && !(flags & DOPF_F_NO_ROW_SKIP)) ? 1 : 0;
    const int NG = S > 0 ? 256 / p.stoLPS : 1;
    int sto_target = 2048;
    const char *sto_env = exp_env("DOPF_STO_TARGET_ITEMS");
    if (sto_env) sto_target = std::max(1, atoi(sto_env));     // (experiments)
    int schunk = std::max(NG, (S + sto_target - 1) / sto_target);
    schunk = (schunk + NG - 1) / NG * NG;
    // Big copper plates (the storage solve is a launch of its own: config4): as many passes per block as make the launch ONE
    // resident round — 3 blocks of 256 threads per CU at the storage code's register count — instead of several rounds of
    // shorter blocks (the blocks' fixed cost — entry, constants, the block's sums — is paid per block, and a round's last
    // blocks leave wave slots idle): config4 1 421 items of 2 passes -> 711 of 4: 78.7 -> 76.8 us per iteration. Only when that
    // round is well filled (a half-empty round of long blocks loses: 569 blocks of 5 passes 84.3 us).
    if (!p.fuseAgents && L == 0 && N == 1 && S > 0 && !sto_env) {
        const int slots = 3 * (cus > 0 ? cus : 256) - 8, units = (S + NG - 1) / NG;
        const int passes = (units + slots - 1) / slots;
        if (passes >= 2 && (units + passes - 1) / passes >= (slots * 4) / 5) schunk = std::max(schunk, passes * NG);
    }
    if (p.stoLong) schunk = 1;         // the long body: one block per storage
    p.stoItem = schunk;
    Layout lo;                         // the cut and the rows make_layout will make
    place_items(sh, p.genItem, p.stoItem, p.fuseNet, lo);
    p.nGenItems = (int)lo.gen_items.size();
    p.nStoItems = (int)lo.sto_items.size();
    p.rowsT = lo.rowsT;                // rows of the transposed partial sums per timestep (networks)
    if (p.fuseAgents && N == 1 && !p.genSkip && chunk <= kGenStreamRows * p.genR2) {
        // as many generator blocks as find a wave slot next to the storage blocks (3 blocks of 256 per CU at the fused
        // kernel's register count): all resident from the start; at least a quarter of the chip
        int nb = 3 * 256 - p.nStoItems - (p.tail ? 1 : 0);        // (tail in the launch: one slot for the tail block)
        if (const char *e = exp_env("DOPF_GEN_BLOCKS")) nb = atoi(e);          // (experiments)
        p.genBlocks = std::min(p.nGenItems, std::max(nb, 192));
    }
    if ((p.nGenItems + p.nStoItems) / kAccRep + 2 > 1000) p.tail = false;     // (the 10-bit arrival count of a replica slot)

    // the consensus step
    const size_t NT = (size_t)N * T, LT = (size_t)L * T, n1 = std::max(NT, LT);
    if (p.wideNet) p.consensus = Consensus::Wide;
    else if (n1 <= kSmallConsensus) p.consensus = Consensus::Small;
    else if (L > 0 && L <= 256 && N <= 256) p.consensus = Consensus::T1024;
    else if ((size_t)std::max(N, 3 * L) * sizeof(double) <= 48 * 1024) p.consensus = Consensus::DualT;
    else p.consensus = Consensus::Generic;
    p.sliceDual = p.consensus == Consensus::Small && NT <= 256;       // k_dual_price_small: 8 chunks of 32 entries
    if (p.consensus == Consensus::T1024) {
        // networks whose dual step is the one-launch kernel: it builds the tables too, with as many waves as find LDS scratch
        // (<= 8) next to its own ~30 KB
        const size_t per_wave = (4 * (size_t)(2 * L) + 1) * sizeof(double), own = 25 * 1024 + (4 * (size_t)N + 3 * (size_t)L) * sizeof(double);
        p.tablesInDual = (int)std::min<size_t>(8, (128 * 1024 - std::min<size_t>(own, 128 * 1024)) / per_wave);
        // the same kernel forms the slack sums of its timestep (see DevView::slackInDual); DOPF_F_NO_TAIL_FUSE keeps the
        // k_reduce launch (the chain a sharded context runs: bitwise comparisons against it)
        p.slackDual = !(flags & DOPF_F_NO_TAIL_FUSE);
    }
    // ... and, while no line is flagged, the node sums too (the quiet chain: no k_slack launch; DevView::quiet, dopf_iterate)
    // (up to 32 rows per node: one batch of the eight lanes' four loads. configs[3] at full size has 25 and is where the gain
    // ends — the node sums cost the dual kernel what k_slack and its boundary cost, 119.3 us per iteration either way)
    p.quiet = p.slackDual && !(flags & (DOPF_F_KEEP_DELTAS | DOPF_F_NO_QUIET)) && quiet_rows_fit(p.rowsT);
    // the same chain on a peer exchange (k_slack stays: its node sums are what is exchanged): a function of the problem's shape and
    // the flags only — every rank decides alike
    p.commQuiet = p.slackDual && !(flags & (DOPF_F_KEEP_DELTAS | DOPF_F_NO_QUIET));

    // every launch family has kernels for a prefix of kStoPairs (kernels_agents.hip: with_sto_pair)
    if (S > 0 && !p.stoLong) {
        int at = 0;
        while (at < kAllPairs && !(kStoPairs[at][0] == p.stoLPS && kStoPairs[at][1] == p.stoNCH)) ++at;
        if (at >= ((p.fuseAgents || p.fuseNet) ? kFusedPairs : kAllPairs))
            if (!p.refusal) p.refusal = "no storage kernel is instantiated for this horizon and chain";
    }
    return p;
}

// Everything of a context's layout that follows from the shape and the plan (see Layout)
inline Layout make_layout(const Shape &sh, const Plan &p)
{
    const int N = sh.N, L = sh.L, T = sh.T;
    Layout lo;
    place_items(sh, p.genItem, p.stoItem, p.fuseNet, lo);
    // level-1 reduce blocks per node: ~16 items per block, at most 64 (and N*RB blocks in total)
    int max_items = 1;
    for (int n = 0; n < N; ++n)      // storage items: scan + warm rows; generators: items, or (one node, streaming) blocks
        max_items = std::max(max_items, (p.genBlocks > 0 ? p.genBlocks : lo.node_gitem_beg[n + 1] - lo.node_gitem_beg[n]) +
                                            2 * (lo.node_sitem_beg[n + 1] - lo.node_sitem_beg[n]));
    lo.reduceRB = std::max(1, std::min(64, (max_items + 31) / 32));
    // Networks: nodes x timestep chunks already give hundreds of blocks, and more than one block per node means the
    // two-level sum — an agent-scope release (a write-back of the XCD's L2) and a ticket in EVERY block. configs[3] at full
    // size has a node with 36 partial rows: 2 blocks per node, 1 416 releases, k_reduce 38 us instead of 9. One block per
    // node walks up to 128 rows (four passes of its 8 x 4 loads in flight) before a second one is worth its ticket.
    if ((long long)N * ((T + 31) / 32) >= 128) lo.reduceRB = std::max(1, std::min(64, (max_items + 127) / 128));
    // dynamic LDS of k_dual_price_t1024, in doubles: q[N] | d[L] | G[L] | S[L] | the rows of its timestep (quiet chain), later the
    // tables' scratch | sd[N] win[N] na[N]
    const size_t scratch = (size_t)p.tablesInDual * (4 * (size_t)(2 * L) + 1);
    lo.dualRowsOff = N + 3 * L;
    lo.dualSdOff = lo.dualRowsOff + (int)std::max(scratch, (size_t)(quiet_rows_fit(lo.rowsT) ? lo.rowsN : 0));
    lo.dualLdsBytes = (int)(((size_t)lo.dualSdOff + 3 * (size_t)N) * sizeof(double));
    return lo;
}

}  // namespace dopf
