// The program tests/test_plan_chain.py builds (g++, address and undefined-behaviour sanitizers) and runs: csrc/dopf_plan.h alone.
// stdin, one case per line:  N L T G S flags cus ki kc  gen_at[0..N)  sto_at[0..N)
// stdout, one line per case: every Plan field, the layout's scalars, and an FNV-1a hash of the items, the node ranges and the rows.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dopf_plan.h"

using namespace dopf;

static uint64_t g_hash;
static void mix(int x)
{
    for (int k = 0; k < 4; ++k) { g_hash ^= (uint64_t)((unsigned)x >> (8 * k) & 0xffu); g_hash *= 1099511628211ull; }
}
static void mix(const std::vector<int> &a)
{
    mix((int)a.size());
    for (int x : a) mix(x);
}
static void mix(const std::vector<Item> &a)
{
    mix((int)a.size());
    for (const Item &it : a) { mix(it.a0); mix(it.a1); mix(it.node); mix(it.row); }
}

int main()
{
    Shape sh{};
    unsigned flags;
    int cus;
    while (scanf("%d %d %d %d %d %u %d %d %d", &sh.N, &sh.L, &sh.T, &sh.G, &sh.S, &flags, &cus, &sh.ki, &sh.kc) == 9) {
        sh.gen_at.assign(sh.N, 0);
        sh.sto_at.assign(sh.N, 0);
        for (int &x : sh.gen_at) if (scanf("%d", &x) != 1) return 2;
        for (int &x : sh.sto_at) if (scanf("%d", &x) != 1) return 2;
        const Plan p = plan_chain(sh, flags, cus);
        const Layout lo = make_layout(sh, p);
        g_hash = 14695981039346656037ull;
        mix(lo.gen_items); mix(lo.sto_items);
        mix(lo.node_gen_beg); mix(lo.node_sto_beg); mix(lo.node_gitem_beg); mix(lo.node_sitem_beg);
        mix(lo.row_of_pos); mix(lo.pos_of_row);
        printf("refusal=%d stoLPS=%d stoNCH=%d stoLong=%d wideNet=%d consensus=%d sliceDual=%d useWarm=%d stoLean=%d genAvail=%d genQuad=%d "
               "stoE0=%d stoLV=%d stoEff=%d fuseAgents=%d fuseNet=%d tail=%d slackDual=%d quiet=%d commQuiet=%d genTT=%d genR=%d genTT2=%d "
               "genR2=%d genTT256=%d genSkip=%d genBlocks=%d tablesInDual=%d genItem=%d stoItem=%d nGenItems=%d nStoItems=%d rowsT=%d",
               p.refusal ? 1 : 0, p.stoLPS, p.stoNCH, p.stoLong, p.wideNet, (int)p.consensus, (int)p.sliceDual, (int)p.useWarm, (int)p.stoLean,
               (int)p.genAvail, (int)p.genQuad, (int)p.stoE0, p.stoLV, (int)p.stoEff, (int)p.fuseAgents, (int)p.fuseNet, (int)p.tail,
               (int)p.slackDual, (int)p.quiet, (int)p.commQuiet, p.genTT, p.genR, p.genTT2, p.genR2, p.genTT256, p.genSkip, p.genBlocks,
               p.tablesInDual, p.genItem, p.stoItem, p.nGenItems, p.nStoItems, p.rowsT);
        printf(" | rowsN=%d rowsT=%d maxNodeAgents=%d reduceRB=%d dualRowsOff=%d dualSdOff=%d dualLdsBytes=%d hash=%016llx\n", lo.rowsN, lo.rowsT,
               lo.maxNodeAgents, lo.reduceRB, lo.dualRowsOff, lo.dualSdOff, lo.dualLdsBytes, (unsigned long long)g_hash);
    }
    return 0;
}
