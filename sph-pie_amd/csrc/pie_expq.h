// pie_expq.h — the expired queue WHILE SCANS AND BATCHES ARE IN FLIGHT (pie_expired_queue_begin / _finish): an order-preserving
// compaction of the rows with prev_now < end <= now that needs no table-sized staging.  gfx950, wave64.  Included by
// pie_scan.hip behind pie_kernels.h; the geometry is pie_expq_plan.h's.
//
// Form: count, prefix, write — no wave ever waits for another.
//   k_expq_pass<KEYED, false>   every wave takes units grid-stride and leaves one count per unit
//   k_block_prefix_wide         one block turns the (at most 16 384) counts into offsets; a counting pass ends here and this
//                               kernel publishes the length
//   k_expq_pass<KEYED, true>    the same walk; a hit is stored at offset[unit] + its rank in the unit (ballot + mbcnt), never at
//                               or past `cap`; the block that finishes last publishes the length
// The predicate column is pie_expired_queue's: the 2-byte liveness key with the full `end` compare on the two boundary keys
// when the derived columns are in step (2 B/row, read twice), the `end` column otherwise (8 B/row, read twice).
// The length reaches the host through mapped pinned memory, sequence word last, as k_block_prefix_wide publishes `m`.
#ifndef PIE_EXPQ_H
#define PIE_EXPQ_H

#include "pie_expq_plan.h"
#include "pie_kernels.h"

namespace pie {

static_assert(kExpqStepRows == kKeyRowsPerLoad * 2, "a step is two key loads per lane");
static_assert(kExpqStepRows == kUnitRows * 8, "a step is eight end loads per lane");
static_assert(kExpqWaves * kWave == 256, "the pass runs 256-thread blocks");

struct ExpqCtl {
    unsigned int done; // blocks of the write pass that have stored everything; the last one publishes and zeroes it
    unsigned int pad[3];
};

// One unit [w0, w1) by one wave.  COUNT form: returns the hits.  WRITE form: stores them in row order from `base` on.
template <bool KEYED, bool WRITE>
__device__ __forceinline__ int expq_unit(const lkey_t* __restrict__ key, const long long* __restrict__ end, long long w0, long long w1,
                                         long long prev_now, long long now, unsigned kp, unsigned kn, long long base, int* __restrict__ queue,
                                         long long cap, const int* __restrict__ row_map, int lane)
{
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    int fill = 0; // wave-uniform
    auto emit = [&](long long pos, long long r) {
        if (pos < cap) queue[pos] = row_map ? row_map[r] : (int)r;
    };
    auto end_hit = [&](long long r) -> bool {
        const long long ev = end[r];
        return (ev <= now) & (ev > prev_now);
    };
    auto key_hit = [&](unsigned k, long long r) -> bool {
        if (k > kp && k < kn) return true;
        if (k != kp && k != kn) return false;
        return end_hit(r);
    };
    const unsigned kp2 = kp | (kp << 16), kn2 = (kn | (kn << 16)) | 0x80008000u;
    for (long long t = w0; t < w1; t += kExpqStepRows) {
        if (t + kExpqStepRows <= w1) {
            if constexpr (KEYED) {
                u4_t kv[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) kv[j] = stream_load<true>(reinterpret_cast<const u4_t*>(key + t + j * kKeyRowsPerLoad + 8 * lane));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // candidates: kp <= key <= kn, per 16-bit half (keys < 2^15: neither subtraction borrows across halves)
                    const unsigned w[4] = {kv[j].x, kv[j].y, kv[j].z, kv[j].w};
                    unsigned cand = 0; // bit q = row q of this lane's eight
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned g = ((w[i] | 0x80008000u) - kp2) & (kn2 - w[i]) & 0x80008000u;
                        cand |= (((g >> 15) & 1u) | ((g >> 30) & 2u)) << (2 * i);
                    }
                    if (__ballot(cand != 0) == 0) continue;
                    const long long r0 = t + j * kKeyRowsPerLoad + 8 * lane;
                    unsigned hits = 0;
                    for (unsigned m = cand; m; m &= m - 1) {
                        const int q = __ffs((int)m) - 1;
                        const unsigned ww = q < 4 ? (q < 2 ? kv[j].x : kv[j].y) : (q < 6 ? kv[j].z : kv[j].w); // no dynamic register indexing
                        const unsigned k = (ww >> ((q & 1) * 16)) & 0xFFFFu;
                        if (key_hit(k, r0 + q)) hits |= 1u << q;
                    }
                    // each lane holds eight consecutive rows, so lane order is row order: exclusive prefix of the lanes' hit counts
                    const int c = __popc(hits);
                    int incl = c;
#pragma unroll
                    for (int o = 1; o < kWave; o <<= 1) {
                        const int v = __shfl_up(incl, o, kWave);
                        if (lane >= o) incl += v;
                    }
                    if constexpr (WRITE) {
                        long long pos = base + fill + incl - c;
                        for (unsigned m = hits; m; m &= m - 1) emit(pos++, r0 + (__ffs((int)m) - 1));
                    }
                    fill += __shfl(incl, kWave - 1, kWave);
                }
            } else {
                ll2_t e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) e[j] = stream_load<true>(reinterpret_cast<const ll2_t*>(end + t + j * kUnitRows + 2 * lane));
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool h0 = (e[j].x <= now) & (e[j].x > prev_now);
                    const bool h1 = (e[j].y <= now) & (e[j].y > prev_now);
                    const unsigned long long b0 = __ballot(h0), b1 = __ballot(h1);
                    if ((b0 | b1) == 0) continue;
                    if constexpr (WRITE) {
                        const long long r = t + j * kUnitRows + 2 * lane;
                        const long long pos = base + fill + prefix_in_ballot(b0) + prefix_in_ballot(b1); // rows 2l, 2l+1 are adjacent
                        if (h0) emit(pos, r);
                        if (h1) emit(pos + (h0 ? 1 : 0), r + 1);
                    }
                    fill += __popcll(b0) + __popcll(b1);
                }
            }
        } else { // the ragged end of the table: 64 rows at a time
            for (long long r0 = t; r0 < w1; r0 += kWave) {
                const long long r = r0 + lane;
                bool h = false;
                if (r < w1) {
                    if constexpr (KEYED) h = key_hit(key[r], r);
                    else h = end_hit(r);
                }
                const unsigned long long b = __ballot(h);
                if constexpr (WRITE) {
                    if (h) emit(base + fill + prefix_in_ballot(b), r);
                }
                fill += __popcll(b);
            }
        }
    }
    return fill;
}

// WRITE = false: unit_count[u] = hits of unit u.  WRITE = true: the hits of unit u go to queue[unit_off[u] ..), below `cap` only;
// unit_off[n_units] is the length, which the block that finishes last hands to the host (host->s.m, then host->seq = seq).
template <bool KEYED, bool WRITE>
__global__ __launch_bounds__(256) void k_expq_pass(const lkey_t* __restrict__ key, const long long* __restrict__ end, long long n,
                                                   long long rows_per_unit, int n_units, long long prev_now, long long now, unsigned kp,
                                                   unsigned kn, int* __restrict__ unit_count, const long long* __restrict__ unit_off,
                                                   int* __restrict__ queue, long long cap, const int* __restrict__ row_map, ExpqCtl* ctl,
                                                   HostSummary* host, unsigned long long seq)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int stride = (int)gridDim.x * kExpqWaves;
    for (int u = (int)blockIdx.x * kExpqWaves + wave; u < n_units; u += stride) {
        const long long w0 = (long long)u * rows_per_unit;
        long long w1 = w0 + rows_per_unit;
        if (w1 > n) w1 = n;
        long long base = 0;
        if constexpr (WRITE) base = unit_off[u];
        const int fill = expq_unit<KEYED, WRITE>(key, end, w0, w1, prev_now, now, kp, kn, base, queue, cap, row_map, lane);
        if constexpr (!WRITE) {
            if (lane == 0) unit_count[u] = fill;
        }
    }
    if constexpr (WRITE) {
        __syncthreads(); // every wave of this block has issued its stores
        if (threadIdx.x == 0) {
            __threadfence();
            const unsigned int before = atomicAdd(&ctl->done, 1u);
            if (before == gridDim.x - 1) { // every block has finished: nothing reads the table any more
                __hip_atomic_store(&ctl->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ready for the next pass
                host->s.m = (unsigned long long)unit_off[n_units];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&host->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

} // namespace pie

#endif
