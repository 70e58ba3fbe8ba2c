// gkm_minimizer_host.h -- the pieces of gk_minimizers / gk_select_minimizers (gkm_minimizer.hip) that
// need no device: the order hash, the canonical key, the local selection rule over an array of ords,
// the two-sided chunk arithmetic and the chunk knob's value (the definition: include/gkm.h).
// Plain C++ outside hipcc (GKM_HD, gkm_canon.h), so that a stand-alone driver can run the kernel's own
// rule under the host sanitizers (tests/sanitize/minimizer_driver.cpp).
#pragma once

#include <stdint.h>

#include "gkm_canon.h"
#include "gkm_query_host.h"

namespace gkm {
namespace minimizer {

constexpr uint32_t kMaxK = 32, kMaxW = 256;
constexpr uint32_t kFlagCanonical = 1u, kFlagLex = 2u;  // GK_MINIMIZER_CANONICAL, GK_MINIMIZER_LEX

// what a position's flag byte says (the kernel's LDS table and the driver's arrays)
constexpr uint8_t kValid = 1;     // a valid start
constexpr uint8_t kStrand = 2;    // its canonical key is the reverse complement's
constexpr uint8_t kSeqStart = 4;  // a sequence starts at this byte: no window crosses to its left

GKM_HD uint64_t fmix64(uint64_t h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
GKM_HD uint64_t mix(uint64_t x) { return fmix64(x ^ 0x9E3779B97F4A7C15ull); }

// reverse complement of the k right-aligned 2-bit symbols of key (1 <= k <= 32)
GKM_HD uint64_t revcomp_key(uint64_t key, int k) {
    uint64_t y = ~key;  // complement: 3 - code
    y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
    y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
    y = __builtin_bswap64(y);
    return y >> (64 - 2 * k);
}

// ckey and strand of a k-mer from its key and its reverse complement's
GKM_HD uint64_t canonical_key(uint64_t key, uint64_t rc, bool canonical, uint32_t *strand) {
    const bool rev = canonical && rc < key;
    *strand = rev ? 1u : 0u;
    return rev ? rc : key;
}
GKM_HD uint64_t ord_of(uint64_t ckey, bool lex) { return lex ? ckey : mix(ckey); }

// The local rule at index i of n positions: selected iff valid and L + R + 1 >= w, L the consecutive
// valid left neighbours of the same sequence with a greater ord, R the consecutive valid right
// neighbours with a greater or equal ord, both capped at w - 1.  Early exit: O(1) expected on random
// data, O(w) per position inside tied or monotone stretches.
GKM_HD bool selected(const uint64_t *ord, const uint8_t *flag, int i, int n, int w) {
    if (!(flag[i] & kValid)) return false;
    const uint64_t o = ord[i];
    int L = 0, q = i;
    while (L < w - 1 && q > 0 && !(flag[q] & kSeqStart) && (flag[q - 1] & kValid) && ord[q - 1] > o) {
        --q;
        ++L;
    }
    const int need = w - 1 - L;
    int R = 0;
    q = i;
    while (R < need && q + 1 < n && (flag[q + 1] & (kValid | kSeqStart)) == kValid && ord[q + 1] >= o) {
        ++q;
        ++R;
    }
    return R >= need;
}

// positions a chunk owns: bounds the device scratch (the chunk's bytes and one count per tile) and
// the pinned staging; GKM_MINIMIZER_CHUNK can lower it (query::knob_below), any value from 1 on
constexpr uint64_t kChunkPositions = 16ull << 20;
inline uint64_t chunk_positions(const char *value) { return query::knob_below(value, kChunkPositions); }

// Chunk i of a batch of `total` bytes owns the positions [own_lo, own_lo + own_n), `step` of them but
// for the last chunk, and carries the bytes [held_lo, held_lo + held_n): w - 1 more on the left, so
// that L of every owned position is decided, and w - 1 + k - 1 more on the right, R's neighbours and
// their k-mers (fewer where the batch ends first).  Every position is owned exactly once.
inline uint64_t chunk_count(uint64_t total, uint64_t step) { return total / step + (total % step != 0); }
inline uint64_t halo_left(uint32_t w) { return w - 1; }
inline uint64_t halo_right(uint32_t k, uint32_t w) { return (uint64_t)(w - 1) + (k - 1); }
inline void chunk_range(uint64_t total, uint64_t step, uint32_t k, uint32_t w, uint64_t i, uint64_t *own_lo,
                        uint64_t *own_n, uint64_t *held_lo, uint64_t *held_n) {
    *own_lo = i * step;
    const uint64_t left = total - *own_lo;
    *own_n = left < step ? left : step;
    *held_lo = *own_lo < halo_left(w) ? 0 : *own_lo - halo_left(w);
    const uint64_t own_hi = *own_lo + *own_n;
    const uint64_t held_hi = total - own_hi < halo_right(k, w) ? total : own_hi + halo_right(k, w);
    *held_n = held_hi - *held_lo;
}
// bytes of the largest chunk: what the scratch and the staging hold
inline uint64_t chunk_bytes_max(uint64_t total, uint64_t step, uint32_t k, uint32_t w) {
    const uint64_t most = step + halo_left(w) + halo_right(k, w);
    return total < most ? total : most;
}

}  // namespace minimizer
}  // namespace gkm
