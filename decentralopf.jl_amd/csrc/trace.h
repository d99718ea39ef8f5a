// trace.h — k_trace: the iteration history on the device (dopf_trace_*). Included by dopf_api.hip alone.
//
// While a trace is active every iteration of dopf_iterate ends with one launch of k_trace, which copies the selected state into
// a slot of the context's ring (trace_layout.h). The slot comes from Status::iters_total, so an iteration that computed nothing
// (halted, capped, parked by the quiet chain) rewrites the slot of the last computed one with the bytes it already holds: no
// word says "seen", and no block waits for another.
#pragma once

#include "dopf_internal.h"
#include "trace_layout.h"

namespace dopf {

struct TraceSeg {
    const double *src;              // a device array of the context
    unsigned long long off, n;      // bytes from the slot's start; doubles
};

// The trace block in device memory: base in front (dopf_trace_begin and dopf_trace_reset write it in order on the context's
// stream; the graphs keep reading this address), then the segment table — the selected, non-empty sections only.
struct TraceBlock {
    int base;                       // Status::iters_total when the trace began or was reset
    int nseg;
    unsigned long long ubeg[kTraceSections + 1];    // 16-byte units in front of segment k; ubeg[nseg]: all of them
    TraceSeg seg[kTraceSections];
};

struct TraceView {
    const Status *st;
    const TraceBlock *blk;
    char *ring;
    int capacity;
    unsigned long long slot_bytes, units;
};

typedef double trace_d2 __attribute__((ext_vector_type(2)));
typedef int trace_i4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_trace(TraceView tv)
{
    __shared__ TraceSeg seg[kTraceSections];
    __shared__ unsigned long long ubeg[kTraceSections + 1];
    const Status *st = tv.st;
    const int rec = st->iters_total - tv.blk->base;
    if (rec <= 0) return;           // nothing computed since begin / reset (uniform: every thread reads the same two words)
    const int nseg = tv.blk->nseg;
    if ((int)threadIdx.x < nseg) seg[threadIdx.x] = tv.blk->seg[threadIdx.x];
    if ((int)threadIdx.x <= nseg) ubeg[threadIdx.x] = tv.blk->ubeg[threadIdx.x];
    char *slot = tv.ring + (size_t)trace_slot(rec, tv.capacity) * tv.slot_bytes;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the residuals may sit as bit patterns (Status::res_set), decoded as read_status does
        const int set = st->res_set, conv = st->converged;
        double r[3];
        for (int k = 0; k < 3; ++k) r[k] = (set == 0 || set == 1) ? __longlong_as_double((long long)st->resbits2[set][k]) : st->res[k];
        const trace_d2 a = {r[0], r[1]}, b = {r[2], st->total_cost};
        const trace_i4 c = {conv ? st->iteration : st->iteration - 1, conv, 0, 0}, z = {0, 0, 0, 0};
        *reinterpret_cast<trace_d2 *>(slot) = a;
        *reinterpret_cast<trace_d2 *>(slot + 16) = b;
        *reinterpret_cast<trace_i4 *>(slot + 32) = c;
        *reinterpret_cast<trace_i4 *>(slot + 48) = z;
    }
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    int k = 0;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < tv.units; u += stride) {
        while (u >= ubeg[k + 1]) ++k;               // (u < units = ubeg[nseg]: k stays below nseg)
        const TraceSeg s = seg[k];
        const unsigned long long j = 2 * (u - ubeg[k]);             // the unit's first double
        double *dst = reinterpret_cast<double *>(slot + s.off) + j;
        // a section starts on a 16-byte boundary of the slot; so does every array of the context. A source off by 8 bytes goes
        // double by double, and so does the last double of an odd section.
        const bool aligned = (reinterpret_cast<uintptr_t>(s.src) & 15) == 0;
        if (aligned && j + 1 < s.n) {
            const trace_d2 x = *reinterpret_cast<const trace_d2 *>(s.src + j);
            __builtin_nontemporal_store(x, reinterpret_cast<trace_d2 *>(dst));      // written once, read later by the host
        } else {
            __builtin_nontemporal_store(s.src[j], dst);
            if (j + 1 < s.n) __builtin_nontemporal_store(s.src[j + 1], dst + 1);
        }
    }
}

// the table of a context's trace: the selected, non-empty sections of the layout and their sources
inline void trace_fill_block(TraceBlock *b, const TraceLayout &lay, const DevView &v, int base)
{
    const double *src[kTraceSections] = {v.lam, v.mu, v.rho, v.inj, v.avgU, v.avgK, v.flow, v.P, v.D, v.C};
    *b = TraceBlock{};
    b->base = base;
    for (int k = 0; k < kTraceSections; ++k) {
        if (lay.n[k] == 0) continue;
        b->seg[b->nseg] = TraceSeg{src[k], (unsigned long long)lay.off[k], (unsigned long long)lay.n[k]};
        b->ubeg[b->nseg + 1] = b->ubeg[b->nseg] + (lay.n[k] + 1) / 2;
        ++b->nseg;
    }
}

// one launch behind the iteration's last kernel. The grid comes from the slot's bytes: a thread moves about four 16-byte units, so
// the three-node case is one block, and a big slot gets enough blocks to keep every CU streaming (grid-stride beyond 1024 blocks).
inline void launch_trace(const TraceView &tv, hipStream_t s)
{
    const unsigned long long want = (tv.units + 1023) / 1024;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 1024 ? 1024 : want);
    hipLaunchKernelGGL(k_trace, dim3(blocks), dim3(256), 0, s, tv);
}

}  // namespace dopf
