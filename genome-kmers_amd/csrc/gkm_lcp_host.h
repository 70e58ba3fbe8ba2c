// gkm_lcp_host.h -- the two comparisons behind gk_lcp (gkm_lcp.hip) and the tile constants its
// kernels share with the tests.  Plain C++ outside hipcc: GKM_HD (as gkm_canon.h's) is __host__ __device__ under hipcc
// only, so the kernels and a stand-alone driver under the host sanitizers
// (tests/sanitize/lcp_driver.cpp) run the same code.
//
// lcp of two adjacent sorted k-mers at a cap: the largest k in 0..cap at which they compare equal
// under sba_equal (gkm_group.hip; kmers.py:306-397) at kmer_len = k.  A '$' on both sides at the same
// offset, after equal bytes, makes them equal at every length (cap); a '$' on one side ends the common
// prefix there.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GKM_HD __host__ __device__ __forceinline__
#else
#define GKM_HD inline
#endif
#include <stdint.h>

namespace gkm {
namespace lcp {

// sorted positions per block and step of every kernel of gkm_lcp.hip: 256 threads x 4, position
// tile0 + j * 256 + thread.  The LCP key kernel takes the key of position q - 1 from the lane below
// (lane 0 of a wave loads it: the halo), the pair kernels (spectrum, min_unique) lcp[q + 1] from the
// lane above (lane 63 loads it)
constexpr uint32_t kThreads = 256;
constexpr uint32_t kItems = 4;
constexpr uint32_t kTile = kThreads * kItems;
// bins 0..kLdsBins-1 of each of the spectrum's two histograms are counted in LDS, the bins above in
// global memory
constexpr uint32_t kLdsBins = 1024;
// rounds of the spectrum's wave reduction: in each, the lanes that hold the first active lane's bin
// are counted by one ballot and added by one lane; what is left after kPeelRounds adds per lane
// (0: one LDS atomic per lane and value, group_hist_kernel's pattern).  Chosen by A/B of variant
// builds, 0..4 and 8 rounds at 1e8 31-mers (profiles/lcp/ab_peel.txt): one round is the fastest on a
// random genome (0.34 ms against 0.37 with none and 0.45 with four) and within 2 % of the fastest on
// one where every k-mer has a twin (0.30 against 0.55 with none); 8 rounds: ab_flush_peel.txt
#ifndef GKM_LCP_PEEL_ROUNDS
#define GKM_LCP_PEEL_ROUNDS 1
#endif
constexpr int kPeelRounds = GKM_LCP_PEEL_ROUNDS;
// the largest cap (the spectrum allocates 16 bytes per length)
constexpr uint32_t kMaxCap = 1u << 24;
constexpr uint32_t kNeverUnique = 0xFFFFFFFFu;

// leading zero bits of x != 0
GKM_HD int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// Encoded keys (gkm_internal.h KeySpec with lenbits == 0): `symbols` symbols of `bits` (2 or 4) bits,
// right-aligned in W 64-bit words, a[0] the most significant, so the first symbol's top bit is bit
// bits * symbols - 1 of the W-word integer.  The number of leading symbols a and b share, at most
// min(symbols, cap).  Equal keys never reach clz64.
template <int W>
GKM_HD uint32_t keys_lcp(const uint64_t *a, const uint64_t *b, int bits, int symbols, uint32_t cap) {
    const uint32_t lim = (uint32_t)symbols < cap ? (uint32_t)symbols : cap;
    const int pad = 64 * W - bits * symbols;  // zero bits above the first symbol
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) {
        const uint64_t x = a[w] ^ b[w];
        if (x != 0) {
            const uint32_t same = (uint32_t)(64 * w + clz64(x) - pad) >> (bits == 2 ? 1 : 2);
            return same < lim ? same : lim;
        }
    }
    return lim;
}

// The bytes at sba + a and sba + b: sba_equal's loop, counting.  Reads offsets [0, cap) at most and
// stops at the first '$' on either side, so with the '$' pad after the sequence every read is in bounds.
GKM_HD uint32_t bytes_lcp(const uint8_t *sba, uint64_t a, uint64_t b, uint32_t cap) {
    for (uint32_t t = 0; t < cap; ++t) {
        const uint8_t x = sba[a + t], y = sba[b + t];
        const bool oa = x == 36, ob = y == 36;  // '$'
        if (oa || ob) return oa && ob ? cap : t;
        if (x != y) return t;
    }
    return cap;
}

// the shortest unique length of a k-mer from m = max(lcp[q], lcp[q + 1]), both clamped to cap
GKM_HD uint32_t min_unique_of(uint32_t m, uint32_t cap) { return m < cap ? m + 1 : kNeverUnique; }

}  // namespace lcp
}  // namespace gkm
