// The program tests/test_ramp_budget_host.py builds (g++, address and undefined-behaviour sanitizers) and runs: csrc/ramp_budget.h and
// csrc/dopf_plan.h alone, no HIP.
// stdin, one request per line:
//   plan flags2 N L T G S flags cus ki kc gen_at[0..N) sto_at[0..N)
//        -> "plan genRampBudget=<0|1> genRamp=<0|1> genBudget=<0|1> refusal=<0|1> genTT2=.. fuseAgents=.. fuseNet=.. tail=.. text=<the
//           refusal, ~ for spaces, or ->"
//   row T q up down prev e_min e_max pmax max_rounds cap[T] c[T]      (hexadecimal doubles; inf allowed; prev nan = no anchor)
//        -> "row rc=<ramp_budget_search's> rounds=<n> nu=<hex> x[0] .. x[T-1]" (hexadecimal doubles): the programme's row at the
//           multiplier found (rc = -1: at 0, as the kernel keeps it)
// The candidates' work arrays are laid out as on the device, [slot][lane] with 64 lanes and exactly 5T + 4 slots: an index past a
// lane's share is an index past the allocation.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dopf_plan.h"
#include "ramp_budget.h"

using namespace dopf;

struct HostCap {
    const double *cap;
    double operator()(int t) const { return cap[t]; }
};

struct HostBatch {
    const double *c;
    HostCap cap;
    int T;
    double q, up, down, prev;
    std::vector<double> work;           // [5T + 4][64]
    double phis[kRampBudgetLanes];
    unsigned long long sigs[kRampBudgetLanes];
    bool run(int lane, double nu, double *out, double *phi, unsigned long long *sig)
    {
        const int K = 2 * T + 2;
        const RbSpan y{work.data() + lane, 64}, kx{work.data() + (size_t)T * 64 + lane, 64}, kv{work.data() + ((size_t)T + K) * 64 + lane, 64};
        return ramp_budget_run(c, nu / q, cap, T, q, up, down, prev, y, kx, kv, K, out, phi, sig);
    }
    void eval(int kind, double a, double b, int n)
    {
        for (int j = 0; j < n; ++j)
            if (!run(j, rb_candidate(kind, a, b, j), nullptr, &phis[j], &sigs[j])) phis[j] = std::nan("");
    }
    double phi(int j) const { return phis[j]; }
    unsigned long long sig(int j) const { return sigs[j]; }
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
            std::string text = p.refusal ? p.refusal : "-";
            for (char &ch : text) if (ch == ' ') ch = '~';
            printf("plan genRampBudget=%d genRamp=%d genBudget=%d refusal=%d genTT2=%d fuseAgents=%d fuseNet=%d tail=%d text=%s\n",
                   (int)p.genRampBudget, (int)p.genRamp, (int)p.genBudget, p.refusal ? 1 : 0, p.genTT2, (int)p.fuseAgents, (int)p.fuseNet,
                   (int)p.tail, text.c_str());
        } else if (!strcmp(what, "row")) {
            int T, max_rounds;
            double q, up, down, prev, e_min, e_max, pm;
            if (scanf("%d %la %la %la %la %la %la %la %d", &T, &q, &up, &down, &prev, &e_min, &e_max, &pm, &max_rounds) != 9 || T < 1) return 2;
            std::vector<double> cap, c, x0((size_t)T), x((size_t)T);
            if (!read_doubles(cap, T) || !read_doubles(c, T)) return 2;
            HostBatch bt{c.data(), HostCap{cap.data()}, T, q, std::fmin(up, pm), std::fmin(down, pm), prev,
                         std::vector<double>((size_t)(5 * T + 4) * 64), {}, {}};
            double phi0 = 0.0;
            unsigned long long sig0;
            if (!bt.run(0, 0.0, x0.data(), &phi0, &sig0)) return 3;
            const double off = phi0 > e_max ? phi0 - e_max : e_min - phi0;
            const double first = std::fmax(off / ((double)T * (1.0 / q)), 1e-12), tol = 1e-12 * (1.0 + (double)T * pm);
            double nu = 0.0;
            int rounds = 0;
            const int rc = ramp_budget_search(bt, phi0, e_min, e_max, first, tol, max_rounds, &nu, &rounds);
            x = x0;
            if (rc == 1) {
                double phi;
                unsigned long long sig;
                if (!bt.run(0, nu, x.data(), &phi, &sig)) return 3;
            }
            printf("row rc=%d rounds=%d nu=%a", rc, rounds, rc == 1 ? nu : 0.0);
            for (double v : x) printf(" %a", v);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
