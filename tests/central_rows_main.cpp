// central_rows_main.cpp — csrc/central_rows.h as a host program (tests/test_central_rows_host.py builds it with g++ under the address
// and undefined-behaviour sanitizers). It reads generator rows from stdin, numbers as hexadecimal doubles (inf, -inf, nan as words),
// and prints what one wave of kc_gen_rows forms for the row, the sums in t order:
//   step T mc absH w ru rd prev e_min e_max yQ | pi[T] cap[T] x0[T] yR[T]     ->  step x+[T] yR+[T] yQ+
//   metrics T mc ru rd prev e_min e_max yQ | pi[T] cap[T] x[T] yR[T]          ->  metrics cost rc_term support violation
// The arrays live on the heap with exactly T entries: a read or write beyond a row is the sanitizer's report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "central_rows.h"

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

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        const bool step = !strcmp(cmd, "step");
        if (!step && strcmp(cmd, "metrics")) { fprintf(stderr, "unknown request %s\n", cmd); return 2; }
        int T = 0;
        if (scanf("%d", &T) != 1 || T < 1 || T > 4096) { fprintf(stderr, "bad T\n"); return 2; }
        double mc, absH = 0.0, w = 1.0, ru, rd, prev, e_min, e_max, yQ;
        bool ok = num(&mc);
        if (step) ok = ok && num(&absH) && num(&w);
        ok = ok && num(&ru) && num(&rd) && num(&prev) && num(&e_min) && num(&e_max) && num(&yQ);
        std::unique_ptr<double[]> pi(new double[T]), cap(new double[T]), x0(new double[T]), yR(new double[T]), xb(new double[T]),
            yRn(new double[T]);
        ok = ok && nums(pi.get(), T) && nums(cap.get(), T) && nums(x0.get(), T) && nums(yR.get(), T);
        if (!ok) { fprintf(stderr, "bad row\n"); return 2; }
        const bool ramp = cr_has_ramp(ru, rd, prev), anch = cr_anchored(prev), bud = cr_has_budget(e_min, e_max);
        if (step) {
            printf("step");
            for (int t = 0; t < T; ++t) {
                const double rc = cr_reduced_cost(mc, pi[t], yR[t], t + 1 < T ? yR[t + 1] : 0.0, yQ);
                const double xn = cr_column_step(x0[t], cr_tau(absH, cr_ramp_rows_at(t, T, ramp, anch), bud ? 1 : 0, w), rc, cap[t]);
                xb[t] = 2.0 * xn - x0[t];
                printf(" %a", xn);
            }
            double sum = 0.0;
            for (int t = 0; t < T; ++t) {
                sum += xb[t];
                yRn[t] = 0.0;
                if (ramp && (t >= 1 || anch))
                    yRn[t] = cr_prox(yR[t], cr_sigma_ramp(t, w), t >= 1 ? xb[t] - xb[t - 1] : xb[t], cr_ramp_lo(t, rd, prev), cr_ramp_hi(t, ru, prev));
                printf(" %a", yRn[t]);
            }
            printf(" %a\n", bud ? cr_prox(yQ, cr_sigma_budget(T, w), sum, e_min, e_max) : 0.0);
        } else {
            double cost = 0.0, rct = 0.0, sup = 0.0, viol = 0.0, sum = 0.0;
            for (int t = 0; t < T; ++t) {
                const double rc = cr_reduced_cost(mc, pi[t], yR[t], t + 1 < T ? yR[t + 1] : 0.0, yQ);
                cost += mc * x0[t];
                rct += cr_rc_term(rc, cap[t]);
                sum += x0[t];
            }
            for (int t = 0; t < T; ++t) {
                double s = 0.0, vv = 0.0;
                if (ramp && (t >= 1 || anch)) {
                    const double lo = cr_ramp_lo(t, rd, prev), hi = cr_ramp_hi(t, ru, prev);
                    s = cr_support(yR[t], lo, hi);
                    vv = cr_violation(t >= 1 ? x0[t] - x0[t - 1] : x0[t], lo, hi);
                }
                sup += s;
                viol = vv > viol ? vv : viol;
            }
            if (bud) {
                sup = sup + cr_support(yQ, e_min, e_max);
                const double vv = cr_violation(sum, e_min, e_max);
                viol = vv > viol ? vv : viol;
            }
            printf("metrics %a %a %a %a\n", cost, rct, sup, viol);
        }
    }
    return 0;
}
