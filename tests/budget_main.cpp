// The program tests/test_budget_host.py builds (g++, address and undefined-behaviour sanitizers) and runs: csrc/budget_root.h and
// csrc/dopf_plan.h alone, no HIP.
// stdin, one request per line:
//   plan flags2 N L T G S flags cus ki kc gen_at[0..N) sto_at[0..N)
//        -> "plan genBudget=<0|1> text=<the refusal, ~ for spaces, or -> | <the line tests/plan_chain_main.cpp prints for the case>"
//   root T e_min e_max max_evals then per step: cap m(kinks) xk[max(m,1)] vk[max(m,1)] sl[m + 1]   (hexadecimal doubles; inf allowed)
//        -> "root rc=<budget_root's> evals=<n> nu=<hex> x[0] .. x[T-1]" (hexadecimal doubles): the row's step at the multiplier found
//           (rc = -1: at 0, the clamped step, as the kernel keeps it)
// A step is the increasing piecewise-linear derivative phi_t of the step's objective, as tests/helpers_ramp_net.py writes it:
// x_t(nu) = clip(phi_t^{-1}(-nu), 0, cap_t).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "budget_root.h"
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

struct HostStep {
    double cap;
    std::vector<double> xk, vk, sl;
    // x_t(nu) and its linear piece
    double at(double nu, int &piece) const
    {
        const int m = (int)sl.size() - 1;
        const double want = -nu;
        int j = 0;
        while (j < m && vk[(size_t)j] < want) ++j;
        const int a = j < m ? j : (m > 0 ? m - 1 : 0);
        const double u = xk[(size_t)a] + (want - vk[(size_t)a]) / sl[(size_t)j];
        piece = budget_piece(u, cap, j);
        return u < 0.0 ? 0.0 : (u > cap ? cap : u);
    }
};

static bool read_doubles(std::vector<double> &a, int n)
{
    a.resize((size_t)n);
    for (double &x : a) if (scanf("%la", &x) != 1) return false;
    return true;
}

int main()
{
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "plan")) {
            Shape sh{};
            unsigned flags, flags2;
            int cus;
            if (scanf("%u %d %d %d %d %d %u %d %d %d", &flags2, &sh.N, &sh.L, &sh.T, &sh.G, &sh.S, &flags, &cus, &sh.ki, &sh.kc) != 10) return 2;
            sh.gen_at.assign((size_t)sh.N, 0);
            sh.sto_at.assign((size_t)sh.N, 0);
            for (int &x : sh.gen_at) if (scanf("%d", &x) != 1) return 2;
            for (int &x : sh.sto_at) if (scanf("%d", &x) != 1) return 2;
            const Plan p = plan_chain(sh, flags, cus, flags2);
            const Layout lo = make_layout(sh, p);
            g_hash = 14695981039346656037ull;
            mix(lo.gen_items); mix(lo.sto_items);
            mix(lo.node_gen_beg); mix(lo.node_sto_beg); mix(lo.node_gitem_beg); mix(lo.node_sitem_beg);
            mix(lo.row_of_pos); mix(lo.pos_of_row);
            std::string text = p.refusal ? p.refusal : "-";
            for (char &ch : text) if (ch == ' ') ch = '~';
            printf("plan genBudget=%d text=%s | ", (int)p.genBudget, text.c_str());
            printf("refusal=%d stoLPS=%d stoNCH=%d stoLong=%d wideNet=%d consensus=%d sliceDual=%d useWarm=%d stoLean=%d genAvail=%d genQuad=%d "
                   "stoE0=%d stoLV=%d stoEff=%d fuseAgents=%d fuseNet=%d tail=%d slackDual=%d quiet=%d commQuiet=%d genTT=%d genR=%d genTT2=%d "
                   "genR2=%d genTT256=%d genSkip=%d genBlocks=%d tablesInDual=%d genItem=%d stoItem=%d nGenItems=%d nStoItems=%d rowsT=%d",
                   p.refusal ? 1 : 0, p.stoLPS, p.stoNCH, p.stoLong, p.wideNet, (int)p.consensus, (int)p.sliceDual, (int)p.useWarm, (int)p.stoLean,
                   (int)p.genAvail, (int)p.genQuad, (int)p.stoE0, p.stoLV, (int)p.stoEff, (int)p.fuseAgents, (int)p.fuseNet, (int)p.tail,
                   (int)p.slackDual, (int)p.quiet, (int)p.commQuiet, p.genTT, p.genR, p.genTT2, p.genR2, p.genTT256, p.genSkip, p.genBlocks,
                   p.tablesInDual, p.genItem, p.stoItem, p.nGenItems, p.nStoItems, p.rowsT);
            printf(" | rowsN=%d rowsT=%d maxNodeAgents=%d reduceRB=%d dualRowsOff=%d dualSdOff=%d dualLdsBytes=%d hash=%016llx\n", lo.rowsN, lo.rowsT,
                   lo.maxNodeAgents, lo.reduceRB, lo.dualRowsOff, lo.dualSdOff, lo.dualLdsBytes, (unsigned long long)g_hash);
        } else if (!strcmp(what, "root")) {
            int T, max_evals;
            double e_min, e_max;
            if (scanf("%d %la %la %d", &T, &e_min, &e_max, &max_evals) != 4 || T < 1) return 2;
            std::vector<HostStep> row((size_t)T);
            double steepest = 0.0;
            for (HostStep &s : row) {
                int m;
                if (scanf("%la %d", &s.cap, &m) != 2 || m < 0) return 2;
                const int n = m > 0 ? m : 1;
                if (!read_doubles(s.xk, n) || !read_doubles(s.vk, n) || !read_doubles(s.sl, m + 1)) return 2;
                for (double v : s.sl) steepest = std::fmax(steepest, 1.0 / v);
            }
            auto sum_at = [&](double nu) {
                double sum = 0.0;
                int piece;
                for (const HostStep &s : row) sum += s.at(nu, piece);
                return sum;
            };
            auto probe = [&](double a, double m, double b) {
                double sum = 0.0;
                BudgetSame sm;
                for (const HostStep &s : row) {
                    int pa, pm, pb;
                    s.at(a, pa);
                    sum += s.at(m, pm);
                    s.at(b, pb);
                    sm.add(pa, pm, pb);
                }
                return BudgetProbe{sum, sm.sameA, sm.sameB, sm.atLo, sm.atHi};
            };
            const double phi0 = sum_at(0.0);
            const double off = phi0 > e_max ? phi0 - e_max : e_min - phi0;
            double nu = 0.0;
            int evals = 0;
            const int rc = budget_root(probe, phi0, e_min, e_max, std::fmax(off / (T * steepest), 1e-12), max_evals, &nu, &evals);
            if (rc < 0) nu = 0.0;
            printf("root rc=%d evals=%d nu=%a", rc, evals, nu);
            for (const HostStep &s : row) { int piece; printf(" %a", s.at(nu, piece)); }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
