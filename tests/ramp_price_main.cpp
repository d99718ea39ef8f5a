// csrc/ramp_price.h as a host program (tests/test_ramp_price_host.py builds it under the address and undefined-behaviour sanitizers).
// stdin, one row per line, every number a hexadecimal double (or inf / nan):
//   row T shift q up down prev pm  then per t: x c floor cap
// stdout: "row" and the T multipliers as hexadecimal doubles. The work arrays and the output live in heap blocks of exactly T doubles:
// a write beyond them is the sanitizer's report. "alias" in place of "row": the output array is the centres' own (the in-place form
// k_gen_ramp uses).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ramp_price.h"

namespace {

struct Tab {
    const double *v;
    double operator()(int t) const { return v[t]; }
};

bool number(std::istringstream &in, double &out)
{
    std::string w;
    if (!(in >> w)) return false;
    char *end = nullptr;
    out = std::strtod(w.c_str(), &end);
    return end && *end == 0;
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        int T = 0;
        double shift, q, up, down, prev, pm;
        if (!(in >> kind >> T) || T < 0 || (kind != "row" && kind != "alias")) return 2;
        if (!number(in, shift) || !number(in, q) || !number(in, up) || !number(in, down) || !number(in, prev) || !number(in, pm)) return 2;
        double *x = new double[T], *c = new double[T], *fl = new double[T], *cp = new double[T];
        double *lo = new double[T], *hi = new double[T];
        for (int t = 0; t < T; ++t)
            if (!number(in, x[t]) || !number(in, c[t]) || !number(in, fl[t]) || !number(in, cp[t])) return 2;
        double *a = kind == "alias" ? c : new double[T];
        dopf::ramp_price(x, c, shift, q, Tab{fl}, Tab{cp}, T, up, down, prev, pm, lo, hi, a);
        std::printf("row");
        for (int t = 0; t < T; ++t) std::printf(" %a", a[t]);
        std::printf("\n");
        if (a != c) delete[] a;
        delete[] x; delete[] c; delete[] fl; delete[] cp; delete[] lo; delete[] hi;
    }
    return 0;
}
