// The gen_pmax block of csrc/dopf_internal.h on the CPU (tests/test_gen_budget_price_abi.py): a main of its own around that header,
// built for the host alone. For a list of shapes it prints every accessor's offset from v.gen_pmax, in doubles, and the block's size:
//   budget G T items  min max price  doubles
//   pair   G T items  up down prev min max scratch price  doubles
//   ramp   G T items L  up down prev scratch min_output  doubles
//   view   sizeof(DevView)
#include <cstdio>
#include <vector>

#include "dopf_internal.h"

int main()
{
    using namespace dopf;
    const int shapes[][4] = {{1, 1, 1, 0}, {12, 5, 1, 0}, {12, 130, 3, 0}, {41, 70, 2, 0}, {7, 129, 2, 8}, {30, 600, 2, 0}};
    for (const auto &s : shapes) {
        const int G = s[0], T = s[1], items = s[2], L = s[3];
        // (a block of the pair's size, the largest of the three, so that every pointer formed below points into it)
        std::vector<double> blk(gen_ramp_budget_doubles(G, T, items) + gen_pmax_doubles(G, T, items, true, L));
        DevView v{};
        v.G = G; v.T = T; v.nGenItems = items; v.gen_pmax = blk.data();
        auto off = [&](const double *p) { return (long long)(p - blk.data()); };
        printf("budget %d %d %d  %lld %lld %lld  %zu\n", G, T, items, off(gen_budget_min(v)), off(gen_budget_max(v)),
               off(gen_budget_price(v, false)), gen_budget_doubles(G));
        printf("pair %d %d %d  %lld %lld %lld %lld %lld %lld %lld  %zu\n", G, T, items, off(gen_ramp_up(v)), off(gen_ramp_down(v)),
               off(gen_ramp_prev(v)), off(gen_rb_min(v)), off(gen_rb_max(v)), off(gen_rb_scratch(v)), off(gen_budget_price(v, true)),
               gen_ramp_budget_doubles(G, T, items));
        v.L = L;
        printf("ramp %d %d %d %d  %lld %lld %lld %lld %lld  %zu\n", G, T, items, L, off(gen_ramp_up(v)), off(gen_ramp_down(v)),
               off(gen_ramp_prev(v)), off(gen_ramp_scratch(v)), off(gen_min_output(v)), gen_pmax_doubles(G, T, items, true, L));
    }
    printf("view %zu\n", sizeof(DevView));
    return 0;
}
