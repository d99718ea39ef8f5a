// csrc/central_long.h on the CPU: for every T on the command line, one line per (tile, thread) of the long sweeps' tiling —
//   T tile thread first mask last_slot hand_slot
// first: the thread's first timestep; mask: bit k set where slot k is live; last_slot: the slot of T - 1 if this thread holds it,
// else -1; hand_slot: the slot handed to the next tile if this thread holds it, else -1. Then one line "tiles T n tile thread slot":
// the tile count and where T - 1 lies by the closed forms. tests/test_central_long_host.py compares with its NumPy twin.
#include <cstdio>
#include <cstdlib>

#include "central_long.h"

using namespace dopf;

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        const int T = atoi(argv[a]);
        if (T < 1) return 2;
        const int tiles = cl_tiles(T);
        for (int tile = 0; tile < tiles; ++tile)
            for (int th = 0; th < kClThreads; ++th) {
                const long long f = cl_first(tile, th);
                int last = -1, hand = -1;
                for (int k = 0; k < kClSlots; ++k) {
                    if (cl_live(f, k, T) && cl_is_last(f, k, T)) last = k;
                    if (cl_hands_over(tile, th, k, T)) hand = k;
                }
                printf("%d %d %d %lld %u %d %d\n", T, tile, th, f, cl_live_mask(f, T), last, hand);
            }
        printf("tiles %d %d %d %d %d\n", T, tiles, cl_last_tile(T), cl_last_thread(T), cl_last_slot(T));
    }
    return 0;
}
