// trace_layout.h — where an iteration's record lands in the trace ring of dopf_trace_* (DESIGN.md 5w), as plain C++ (no HIP
// include: tests/test_trace_layout_host.py compiles this header alone, with sanitizers, against a NumPy twin). Host code
// (dopf_trace_begin, dopf_trace_read) and the kernel (k_trace, trace.h) use this one text:
//   trace_layout   the slot: a 64-byte row, then the sections `what` selects, each on a 16-byte boundary
//   trace_slot / trace_held / trace_oldest   the ring arithmetic over `recorded`, the slots written since begin or reset
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DOPF_TRACE_HD __host__ __device__
#else
#define DOPF_TRACE_HD
#endif

namespace dopf {

// the bits of `what` (include/dopf.h: DOPF_TRACE_*)
constexpr int kTraceDuals = 1, kTraceConsensus = 2, kTracePrimal = 4, kTraceKnown = 7;

// The row every slot starts with: what dopf_get_residuals and dopf_get_consensus' total_cost return right after the iteration,
// the value admm.iteration had during that solve, and Convergence.all.
struct TraceRow {
    double res[3];
    double total_cost;
    int32_t iteration, converged;
    int32_t pad[6];
};
constexpr size_t kTraceRowBytes = 64, kTraceAlign = 16;
static_assert(sizeof(TraceRow) == kTraceRowBytes, "the row is 64 bytes");

// the sections behind the row, in slot order; each is the device array of the same name, copied as it lies (P, D, C: sorted order)
enum TraceSec : int { kSecLambda, kSecMu, kSecRho, kSecInj, kSecAvgU, kSecAvgK, kSecFlow, kSecP, kSecD, kSecC, kTraceSections };

struct TraceLayout {
    size_t off[kTraceSections];     // bytes from the slot's start (a multiple of 16); of an absent section: where it would start
    size_t n[kTraceSections];       // doubles; 0: not selected, or empty (G, S or L = 0)
    size_t slot_bytes;              // a multiple of 16
};

// the bit of `what` that selects section k
DOPF_TRACE_HD inline int trace_bit_of(int k) { return k <= kSecRho ? kTraceDuals : k <= kSecFlow ? kTraceConsensus : kTracePrimal; }

DOPF_TRACE_HD inline TraceLayout trace_layout(int N, int L, int T, int G, int S, int what)
{
    const size_t t = (size_t)T, NT = (size_t)N * t, LT = (size_t)L * t;
    const size_t full[kTraceSections] = {t, LT, LT, NT, LT, LT, LT, (size_t)G * t, (size_t)S * t, (size_t)S * t};
    TraceLayout lay{};
    size_t at = kTraceRowBytes;
    for (int k = 0; k < kTraceSections; ++k) {
        lay.off[k] = at;
        lay.n[k] = (what & trace_bit_of(k)) ? full[k] : 0;
        at += (lay.n[k] * sizeof(double) + kTraceAlign - 1) / kTraceAlign * kTraceAlign;
    }
    lay.slot_bytes = at;
    return lay;
}

// recorded >= 1 slots written: the ring slot the last of them went to
DOPF_TRACE_HD inline int trace_slot(long long recorded, int capacity) { return (int)((recorded - 1) % capacity); }
// the slots the ring still holds ...
DOPF_TRACE_HD inline int trace_held(long long recorded, int capacity) { return recorded < capacity ? (int)recorded : capacity; }
// ... and the ring slot of the oldest of them (held slot i lies in ring slot (oldest + i) % capacity)
DOPF_TRACE_HD inline int trace_oldest(long long recorded, int capacity) { return recorded <= capacity ? 0 : (int)(recorded % capacity); }

}  // namespace dopf
