// central_sto_main.cpp — csrc/central_sto.h as a host program (tests/test_central_sto_host.py builds it with g++ under the address and
// undefined-behaviour sanitizers). It reads storage rows from stdin, numbers as hexadecimal doubles, and prints what the storage sweeps
// of kernels_central.hip form for the row, one timestep after the other with sequential prefix and suffix sums:
//   step LV T mc pm em e0 elo ehi al be absH w | pi[T] yE[T] d0[T] c0[T]     ->  step D+[T] C+[T] yE+[T]
//   metrics LV T mc pm em e0 elo ehi al be | pi[T] yE[T] d[T] c[T]           ->  metrics cost rc_term violation support E[T]
// A level LV reads the constants it has (below 1 e0 is 0, below 2 the band is [0, em], below 3 al = be = 1, whatever the line says: the
// kernels' loader). The arrays live on the heap with exactly T entries: a read or write beyond a row is the sanitizer's report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "central_sto.h"

using namespace dopf;

static bool num(double *out)
{
    char tok[64];
    if (scanf("%63s", tok) != 1) return false;
    char *end = nullptr;
    *out = strtod(tok, &end);
    return end != tok && *end == 0;
}

static bool nums(double *a, int n)
{
    for (int i = 0; i < n; ++i)
        if (!num(a + i)) return false;
    return true;
}

struct Row {
    int T;
    StoRow r;
    double absH, w;
    std::unique_ptr<double[]> pi, yE, d0, c0;
};

template <int LV>
static void run(bool step, const Row &in)
{
    const int T = in.T;
    StoRow r = in.r;
    if (LV < 1) r.e0 = 0.0;
    if (LV < 2) { r.elo = 0.0; r.ehi = r.em; }
    if (LV < 3) r.al = r.be = 1.0;
    std::unique_ptr<double[]> dn(new double[T]), cn(new double[T]), out(new double[T]);
    double total = 0.0;
    for (int t = 0; t < T; ++t) total += in.yE[t];
    double before = 0.0, cost = 0.0, dpart = 0.0, yterm = 0.0, viol = 0.0;
    for (int t = 0; t < T; ++t) {
        const double suf = total - before;            // sum_{tau >= t} yE
        before += in.yE[t];
        double rD, rC;
        cs_reduced_costs<LV>(r, in.pi[t], suf, rD, rC);
        if (step) cs_column_steps<LV>(r, in.absH, in.w, T, t, in.d0[t], in.c0[t], rD, rC, dn[t], cn[t]);
        else {
            cost += r.mc * (in.d0[t] + in.c0[t]);
            dpart += cs_rc_term(rD, rC, r.pm);
            yterm = cs_support<LV>(r, in.yE[t], t, T, yterm);
        }
    }
    double lev = 0.0;
    if (LV >= 1) lev += r.e0;
    for (int t = 0; t < T; ++t) {
        if (step) {
            lev += cs_net<LV>(r, cs_extra(dn[t], in.d0[t]), cs_extra(cn[t], in.c0[t]));
            const double sg = cs_sigma<LV>(r, in.w, t);
            out[t] = cs_prox<LV>(r, in.yE[t] + sg * lev, sg, t, T);
        } else {
            lev += cs_net<LV>(r, in.d0[t], in.c0[t]);
            out[t] = lev;
            const double vv = cs_violation<LV>(r, lev, t, T);
            viol = vv > viol ? vv : viol;
        }
    }
    if (step) {
        printf("step");
        for (int t = 0; t < T; ++t) printf(" %a", dn[t]);
        for (int t = 0; t < T; ++t) printf(" %a", cn[t]);
    } else printf("metrics %a %a %a %a", cost, dpart, viol, yterm);
    for (int t = 0; t < T; ++t) printf(" %a", out[t]);
    printf("\n");
}

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        const bool step = !strcmp(cmd, "step");
        if (!step && strcmp(cmd, "metrics")) { fprintf(stderr, "unknown request %s\n", cmd); return 2; }
        int LV = -1;
        Row in;
        in.absH = 0.0;
        in.w = 1.0;
        if (scanf("%d %d", &LV, &in.T) != 2 || LV < 0 || LV > 3 || in.T < 1 || in.T > 4096) { fprintf(stderr, "bad LV or T\n"); return 2; }
        const int T = in.T;
        StoRow &r = in.r;
        bool ok = num(&r.mc) && num(&r.pm) && num(&r.em) && num(&r.e0) && num(&r.elo) && num(&r.ehi) && num(&r.al) && num(&r.be);
        if (step) ok = ok && num(&in.absH) && num(&in.w);
        in.pi.reset(new double[T]); in.yE.reset(new double[T]); in.d0.reset(new double[T]); in.c0.reset(new double[T]);
        ok = ok && nums(in.pi.get(), T) && nums(in.yE.get(), T) && nums(in.d0.get(), T) && nums(in.c0.get(), T);
        if (!ok) { fprintf(stderr, "bad row\n"); return 2; }
        if (LV == 0) run<0>(step, in);
        else if (LV == 1) run<1>(step, in);
        else if (LV == 2) run<2>(step, in);
        else run<3>(step, in);
    }
    return 0;
}
