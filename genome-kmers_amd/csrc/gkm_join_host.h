// gkm_join_host.h -- the index arithmetic of gk_join's key path (gkm_join.hip): the merge-path
// diagonal search, the tile count and the two bounds the tile kernels search their staged slices
// with.  Plain C++ (no HIP include): GKM_JOIN_HD is __host__ __device__ under hipcc and nothing
// elsewhere, so the kernels and a stand-alone driver under the host sanitizers
// (tests/sanitize/join_driver.cpp) run the same code.
//
// The two lists are the unique views of two sorted contexts: list x's element i is the key
// keys_x[heads_x[i]] (heads_x = the group starts, gk_unique_counts; nullptr = the keys as they
// stand), strictly ascending.  No key value is reserved -- 0 and 2^64 - 1 are ordinary keys -- so
// every search runs over explicit lengths and never compares a pad.
//
// Tie rule: in the merged order an element of A precedes the equal element of B.  So for an A element
// at merged position p, every B element before p is strictly smaller and the B element at p + 1, if
// there is one, is its match or greater: a tile that holds A[i0, i1) and B[j0, j1) finds the lower
// bound of each of its A elements inside B[j0, j1] -- its own B slice plus ONE element of the next
// tile (the match of a tile's last A element can be the next tile's first B element).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GKM_JOIN_HD __host__ __device__
#else
#define GKM_JOIN_HD
#endif

namespace gkm {
namespace join {

// merged elements (of A and B together) per tile: 256 threads x 4.  Measured at 1e8 31-mers a side
// (profiles/join/ab_tile.txt): 2048 / 1024 / 512 give 1.46 / 0.97 / 1.09 ms for the tile kernel and
// 0.18 / 0.37 / 0.71 ms for the partition kernel
constexpr uint32_t kTile = 1024;

GKM_JOIN_HD inline uint64_t tile_count(uint64_t na, uint64_t nb) { return (na + nb + kTile - 1) / kTile; }

GKM_JOIN_HD inline uint64_t key_at(const uint64_t *keys, const uint32_t *heads, uint64_t i) {
    return keys[heads ? (uint64_t)heads[i] : i];
}

// The number of A elements among the first d elements of the merged order (0 <= d <= na + nb); the
// first d then hold B[0, d - result).  Every index read lies in [0, na) / [0, nb).
GKM_JOIN_HD inline uint64_t diagonal_split(const uint64_t *ka, const uint32_t *ha, uint64_t na, const uint64_t *kb,
                                           const uint32_t *hb, uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);  // A[mid] against B[d - 1 - mid]: 0 <= d - 1 - mid < nb
        if (key_at(ka, ha, mid) <= key_at(kb, hb, d - 1 - mid)) lo = mid + 1;  // A first on a tie
        else hi = mid;
    }
    return lo;
}

// number of v[0, n) below x (v ascending)
GKM_JOIN_HD inline uint32_t lower_bound_u64(const uint64_t *v, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// number of v[0, n) not above x (v ascending)
template <typename N>
GKM_JOIN_HD inline N upper_bound_u32(const uint32_t *v, N n, uint64_t x) {
    N lo = 0, hi = n;
    while (lo < hi) {
        const N mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace join
}  // namespace gkm
