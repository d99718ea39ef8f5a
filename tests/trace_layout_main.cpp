// csrc/trace_layout.h on the CPU (tests/test_trace_layout_host.py): a main of its own around that header alone. Prints, for a list
// of shapes and every mask, the slot's size and every section's offset and length, and for a few capacities the ring arithmetic:
//   layout N L T G S what slot_bytes (off n) x 10
//   ring capacity recorded slot held oldest          (slot: -1 with nothing recorded)
#include <cstdio>
#include <initializer_list>

#include "trace_layout.h"

int main()
{
    using namespace dopf;
    const int shapes[][5] = {{3, 3, 2, 4, 1}, {3, 3, 2, 4, 0}, {3, 3, 2, 0, 1}, {3, 0, 2, 4, 1}, {3, 3, 5, 4, 1}, {1, 0, 5, 3, 3},
                             {1, 0, 1, 1, 1}, {20, 30, 168, 60, 6}};
    for (const auto &s : shapes)
        for (int what = 0; what < 8; ++what) {
            const TraceLayout lay = trace_layout(s[0], s[1], s[2], s[3], s[4], what);
            printf("layout %d %d %d %d %d %d %zu", s[0], s[1], s[2], s[3], s[4], what, lay.slot_bytes);
            for (int k = 0; k < kTraceSections; ++k) printf(" %zu %zu", lay.off[k], lay.n[k]);
            printf("\n");
        }
    for (int cap : {1, 2, 5, 64}) {
        const long long recs[] = {0, 1, cap - 1, cap, cap + 1, 3LL * cap + 2};
        for (long long r : recs)
            printf("ring %d %lld %d %d %d\n", cap, r, r > 0 ? trace_slot(r, cap) : -1, trace_held(r, cap), trace_oldest(r, cap));
    }
    return 0;
}
