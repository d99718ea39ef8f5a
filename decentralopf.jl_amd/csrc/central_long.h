// central_long.h — who owns which timestep in the long sweeps of the device LP (kc_sto_long, kc_gen_rows_long in kernels_central.hip;
// DESIGN.md 5v): one block of 256 threads walks a row in tiles of 2048 consecutive timesteps (the tile of sto_long.h), thread i owns the
// 8 consecutive steps tile * 2048 + 8 i .. + 7 — consecutive for the reason given above kc_gen_rows: a row that couples t with t - 1
// finds both neighbours in registers but at a thread's two ends.
// Plain C++, no HIP include: the kernels run it on the device, tests/central_long_main.cpp as a host program under sanitizers.
//
//   live slot      its timestep is below T (only the last tile has others; a thread's live slots are a prefix of its 8)
//   slot of T - 1  the one slot the terminal band applies to: tile (T-1) / 2048, thread ((T-1) % 2048) / 8, slot (T-1) % 8
//   hand-over      the last slot of the last thread of every tile but the last one: its value is the left neighbour of the next tile's
//                  first slot (a difference's t - 1), carried as a block-uniform value; that tile is full, so the slot is live
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOPF_CL_FN __host__ __device__ inline
#else
#define DOPF_CL_FN inline
#endif

namespace dopf {

constexpr int kClThreads = 256, kClSlots = 8, kClTile = kClThreads * kClSlots;

// (64-bit: the last tile's dead slots lie past T, which may be close to the largest int)
DOPF_CL_FN int cl_tiles(int T) { return (int)(((long long)T + kClTile - 1) / kClTile); }
DOPF_CL_FN long long cl_first(int tile, int thread) { return (long long)tile * kClTile + (long long)thread * kClSlots; }
DOPF_CL_FN bool cl_live(long long first, int k, int T) { return first + k < (long long)T; }
DOPF_CL_FN unsigned cl_live_mask(long long first, int T)
{
    unsigned m = 0;
    for (int k = 0; k < kClSlots; ++k) m |= cl_live(first, k, T) ? 1u << k : 0u;
    return m;
}

DOPF_CL_FN int cl_last_tile(int T) { return (T - 1) / kClTile; }
DOPF_CL_FN int cl_last_thread(int T) { return ((T - 1) % kClTile) / kClSlots; }
DOPF_CL_FN int cl_last_slot(int T) { return (T - 1) % kClSlots; }
DOPF_CL_FN bool cl_is_last(long long first, int k, int T) { return first + k == (long long)T - 1; }

DOPF_CL_FN bool cl_hands_over(int tile, int thread, int k, int T)
{
    return thread == kClThreads - 1 && k == kClSlots - 1 && tile + 1 < cl_tiles(T);
}

}  // namespace dopf
