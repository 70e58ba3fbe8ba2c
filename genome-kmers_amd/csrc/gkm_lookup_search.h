// gkm_lookup_search.h -- the key path's search, shared by gk_lookup (gkm_lookup.hip), gk_screen
// (gkm_screen.hip) and gk_match (gkm_match.hip): the range of a 2-bit prefix in the sorted one-word
// keys (gfx950).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gkm {

// keys: n one-word keys of `symbols` 2-bit symbols, right-aligned, ascending.  The
// q-symbol prefix of a key is key >> shift with shift = 2 (symbols - q) in [0, 62]: no sum that
// could pass 2^64 (the all-T 32-mer is 2^64 - 1) and no shift by 64.  qb = 2 q.  dir (may be null):
// the directory of the top D key bits (lookup_dir_kernel).  For each of the W prefixes with
// active[w]: first[w] = the number of keys whose prefix is below prefix[w], count[w] = the number
// equal to it; an inactive slot gives 0, 0 and reads nothing.  The W searches advance in lockstep,
// one probe each per round, so a thread keeps W independent gathers in flight; with W = 1 this is
// the plain lower bound followed by the upper bound from it.
template <int W>
__device__ __forceinline__ void key_search(const uint64_t *__restrict__ keys, uint64_t n,
                                           const uint32_t *__restrict__ dir, int D, int qb, int shift,
                                           const uint64_t (&prefix)[W], const bool (&active)[W], uint64_t (&first)[W],
                                           uint32_t (&count)[W]) {
    uint64_t lo[W], hi[W], end[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        lo[w] = 0;
        hi[w] = active[w] ? n : 0;
    }
    if (dir != nullptr) {
        // the two entries that bracket the prefix are the answer (gk_lookup's prefix queries only:
        // gk_screen searches whole keys, qb = 2 * symbols >= D)
        if (qb < D) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                first[w] = 0;
                count[w] = 0;
                if (!active[w]) continue;
                const uint64_t a = dir[prefix[w] << (D - qb)], b = dir[(prefix[w] + 1) << (D - qb)];
                first[w] = a;
                count[w] = (uint32_t)(b - a);
            }
            return;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (!active[w]) continue;
            const uint64_t d = prefix[w] >> (qb - D);
            lo[w] = dir[d];
            hi[w] = dir[d + 1];
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) end[w] = hi[w];
    bool more;
    do {  // keys below the prefix
        more = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (lo[w] >= hi[w]) continue;
            const uint64_t mid = (lo[w] + hi[w]) >> 1;
            if ((keys[mid] >> shift) < prefix[w]) lo[w] = mid + 1;
            else hi[w] = mid;
            more |= lo[w] < hi[w];
        }
    } while (more);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        first[w] = lo[w];
        hi[w] = end[w];
    }
    do {  // ... and not above it, from the lower bound on
        more = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (lo[w] >= hi[w]) continue;
            const uint64_t mid = (lo[w] + hi[w]) >> 1;
            if ((keys[mid] >> shift) <= prefix[w]) lo[w] = mid + 1;
            else hi[w] = mid;
            more |= lo[w] < hi[w];
        }
    } while (more);
#pragma unroll
    for (int w = 0; w < W; ++w) count[w] = (uint32_t)(lo[w] - first[w]);
}

// gk_match's two searches (gkm_match.hip), siblings of key_search over the same keys and directory.
//
// key_lower_bound: pos[w] = the number of keys below the whole key q[w] (kb = 2 * symbols bits, D <= kb),
// the insertion point whose two neighbours decide the longest common prefix; an inactive slot gives 0
// and reads nothing.
template <int W>
__device__ __forceinline__ void key_lower_bound(const uint64_t *__restrict__ keys, uint64_t n,
                                                const uint32_t *__restrict__ dir, int D, int kb,
                                                const uint64_t (&q)[W], const bool (&active)[W], uint64_t (&pos)[W]) {
    uint64_t lo[W], hi[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        lo[w] = 0;
        hi[w] = active[w] ? n : 0;
        if (dir != nullptr && active[w]) {
            const uint64_t d = q[w] >> (kb - D);
            lo[w] = dir[d];
            hi[w] = dir[d + 1];
        }
    }
    bool more;
    do {
        more = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (lo[w] >= hi[w]) continue;
            const uint64_t mid = (lo[w] + hi[w]) >> 1;
            if (keys[mid] < q[w]) lo[w] = mid + 1;
            else hi[w] = mid;
            more |= lo[w] < hi[w];
        }
    } while (more);
#pragma unroll
    for (int w = 0; w < W; ++w) pos[w] = lo[w];
}

// key_search with a prefix length per slot: prefix[w] holds qsym[w] symbols, 1 <= qsym[w] <= symbols
// (kb = 2 * symbols), so qb = 2 qsym[w] and shift = kb - qb in [0, 62] as above, slot by slot.  A slot
// whose prefix is shorter than the directory's D bits is answered by its two entries alone.
template <int W>
__device__ __forceinline__ void key_search_each(const uint64_t *__restrict__ keys, uint64_t n,
                                                const uint32_t *__restrict__ dir, int D, int kb,
                                                const int (&qsym)[W], const uint64_t (&prefix)[W],
                                                const bool (&active)[W], uint64_t (&first)[W], uint32_t (&count)[W]) {
    uint64_t lo[W], hi[W], end[W];
    int shift[W];
    bool done[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int qb = 2 * qsym[w];
        shift[w] = active[w] ? kb - qb : 0;
        lo[w] = 0;
        hi[w] = active[w] ? n : 0;
        first[w] = 0;
        count[w] = 0;
        done[w] = !active[w];
        if (dir == nullptr || !active[w]) continue;
        if (qb < D) {
            const uint64_t a = dir[prefix[w] << (D - qb)], b = dir[(prefix[w] + 1) << (D - qb)];
            first[w] = a;
            count[w] = (uint32_t)(b - a);
            done[w] = true;
            hi[w] = 0;
        } else {
            const uint64_t d = prefix[w] >> (qb - D);
            lo[w] = dir[d];
            hi[w] = dir[d + 1];
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) end[w] = hi[w];
    bool more;
    do {  // keys below the prefix
        more = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (lo[w] >= hi[w]) continue;
            const uint64_t mid = (lo[w] + hi[w]) >> 1;
            if ((keys[mid] >> shift[w]) < prefix[w]) lo[w] = mid + 1;
            else hi[w] = mid;
            more |= lo[w] < hi[w];
        }
    } while (more);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (!done[w]) first[w] = lo[w];
        hi[w] = end[w];
    }
    do {  // ... and not above it, from the lower bound on
        more = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (lo[w] >= hi[w]) continue;
            const uint64_t mid = (lo[w] + hi[w]) >> 1;
            if ((keys[mid] >> shift[w]) <= prefix[w]) lo[w] = mid + 1;
            else hi[w] = mid;
            more |= lo[w] < hi[w];
        }
    } while (more);
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (!done[w]) count[w] = (uint32_t)(lo[w] - first[w]);
}

}  // namespace gkm
