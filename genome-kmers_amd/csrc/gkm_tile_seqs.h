// gkm_tile_seqs.h -- how a block that owns a tile of batch positions finds the sequences they belong
// to, shared by gk_screen (gkm_screen.hip) and gk_match (gkm_match.hip) (gfx950).
//
// A batch is `offsets` (nseq + 1 entries, ascending from 0) over bytes laid back to back.  A tile
// [g0, g1) finds the sequences of its first and last position by a search over `offsets` that the 64
// lanes of one wave share (tile_seq_span), then walks the sequences between them in passes of up to
// BOUNDS (tile_seq_passes): a pass keeps its sequences' ends in LDS, the caller sums per sequence in
// LDS tables of its own and issues one global atomic per (block, sequence) and counter.  A tile with
// more than BOUNDS sequences -- many empty or very short reads -- takes several passes.
// gk_minimizers (gkm_minimizer.hip) uses tile_seq_span alone: it marks the sequence starts between the
// two ends in its staged tile and keeps no table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gkm {

// first u in [lo, hi] with off[u] > g, given off[hi] > g and off[u] <= g for every u < lo; called by
// all 64 lanes of a wave, which probe 64 evenly spaced entries per round
__device__ __forceinline__ uint64_t wave_upper_bound(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi,
                                                     uint64_t g, int lane) {
    while (lo < hi) {
        const uint64_t stride = (hi - lo) / 64 + 1;
        const uint64_t x = lo + (uint64_t)lane * stride;
        const bool above = x >= hi || off[x] > g;
        const unsigned long long m = __ballot(above);
        const int f = m ? __ffsll((long long)m) - 1 : 64;  // the first lane whose entry is above g
        if (f == 0) return lo;
        const uint64_t top = lo + (uint64_t)f * stride;
        lo = lo + (uint64_t)(f - 1) * stride + 1;
        hi = top < hi ? top : hi;
    }
    return lo;
}

// the sequences of the tile's first and last position, g0 and g1 - 1, into s_j[0] and s_j[1] (LDS);
// called by the block's first wave (tid < 64), the block synchronises afterwards
__device__ __forceinline__ void tile_seq_span(const uint64_t *__restrict__ offsets, uint64_t nseq, uint64_t g0,
                                              uint64_t g1, int tid, uint64_t *s_j) {
    const uint64_t u0 = wave_upper_bound(offsets, 0, nseq, g0, tid);
    uint64_t lo = u0, hi = nseq;
    const uint64_t near = u0 + 63 < nseq ? u0 + 63 : nseq;  // (mostly a few sequences on)
    if (offsets[near] > g1 - 1) hi = near;
    else lo = near + 1;
    const uint64_t u1 = wave_upper_bound(offsets, lo, hi, g1 - 1, tid);
    if (tid == 0) {
        s_j[0] = u0 - 1;
        s_j[1] = u1 - 1;
    }
}

// index in the pass of the sequence that holds position pa: the first of the pass's cnt ends above pa
__device__ __forceinline__ int pass_seq_of(const uint64_t *s_tab, int cnt, uint64_t pa) {
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_tab[mid] <= pa) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The passes over the sequences j0..j1 of the tile [g0, g1), called by every thread of a block of
// THREADS.  Per pass over the sequences [ja, ja + cnt): s_tab[i] = the end of sequence ja + i and
// init(i) by the thread that loads it; a barrier; body(ja, cnt, slab_lo, slab_hi) by every thread, the
// pass's positions being [slab_lo, slab_hi); a barrier; flush(i, ja + i) once per sequence.
template <int BOUNDS, int THREADS, class Init, class Body, class Flush>
__device__ __forceinline__ void tile_seq_passes(const uint64_t *__restrict__ offsets, uint64_t j0, uint64_t j1,
                                                uint64_t g0, uint64_t g1, uint64_t *s_tab, int tid, Init init,
                                                Body body, Flush flush) {
    uint64_t ja = j0, slab_lo = g0;
    for (;;) {  // passes of up to BOUNDS sequences
        const uint64_t jb = j1 - ja < (uint64_t)BOUNDS ? j1 : ja + BOUNDS - 1;
        const int cnt = (int)(jb - ja + 1);
        for (int i = tid; i < cnt; i += THREADS) {
            s_tab[i] = offsets[ja + 1 + i];
            init(i);
        }
        __syncthreads();
        const uint64_t last = s_tab[cnt - 1];
        const uint64_t slab_hi = last < g1 ? last : g1;  // the pass's positions: [slab_lo, slab_hi)
        body(ja, cnt, slab_lo, slab_hi);
        __syncthreads();
        for (int i = tid; i < cnt; i += THREADS) flush(i, ja + i);  // one atomic per (block, sequence) and counter
        if (jb == j1) break;
        ja = jb + 1;
        slab_lo = slab_hi;
        __syncthreads();
    }
}

}  // namespace gkm
