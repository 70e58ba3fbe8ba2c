// gkm_match_host.h -- the pieces of gk_match (gkm_match.hip) that are plain C++: the neighbour
// comparison of both paths, the packed (length, first position) word of the per-sequence maximum, the
// cap's range and the chunk size.  GKM_HD (gkm_canon.h) is __host__ __device__ under hipcc only, so the
// kernel and a stand-alone driver under the host sanitizers (tests/sanitize/match_driver.cpp) run the
// same code.
//
// The longest prefix of a query that occurs in a prefix-sorted list is attained next to the query's
// insertion point: every entry that shares l symbols with the query lies in one run of the order, the
// insertion point is inside or at an end of that run, so the predecessor or the successor shares at
// least l.  The search therefore gives the insertion point and these routines the two common prefixes.
#pragma once

#include "gkm_bytes_search.h"
#include "gkm_screen_host.h"

namespace gkm {
namespace match {

// the largest cap after a sort with max_kmer_len None: keeps the C - 1 bytes that consecutive chunks
// share far below a chunk
constexpr uint32_t kMaxCap = 4096;
// bytes of reads per launch, the C - 1 bytes a chunk shares with the next one included.  The
// per-position results are 16 B per byte against gk_screen's 4: at 4 MiB a pinned slot is 68 MiB, below
// the screen's 80 (16 MiB of reads and their counts); GKM_MATCH_CHUNK can lower it
constexpr uint64_t kChunkBytes = 4ull << 20;

// bytes per launch at cap C: kChunkBytes, lowered by the knob, and at least C so that a chunk holds
// one whole match; the chunks themselves are gk_screen's (screen::chunk_step, chunk_count,
// chunk_range) with C in the place of K: an overlap of C - 1 bytes
inline uint64_t chunk_bytes(const char *value, uint32_t C) {
    const uint64_t c = query::knob_below(value, kChunkBytes);
    return c < C ? (uint64_t)C : c;
}

// the cap C of a call: max_len, or the sort length K for 0 after a bounded sort (sort_len != 0);
// 0 when max_len is out of range (above K; 0 or above kMaxCap after None)
inline uint32_t resolve_cap(uint32_t sort_len, uint32_t max_len) {
    if (sort_len != 0) return max_len == 0 ? sort_len : max_len <= sort_len ? max_len : 0;
    return max_len <= kMaxCap ? max_len : 0;
}

// leading zero bits of x != 0
GKM_HD int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// symbols that two keys of K 2-bit symbols (right-aligned, K <= 32) share from the first on
GKM_HD int key_common(uint64_t a, uint64_t b, int K) {
    return a == b ? K : (clz64(a ^ b) - (64 - 2 * K)) >> 1;
}

// Key path: q = the query's m symbols followed by zeros up to K symbols, prev / next = the keys before
// and at q's insertion point where they exist.  The longest prefix of the m symbols that is a prefix
// of a key.
GKM_HD int key_match_len(uint64_t q, int m, uint64_t prev, bool has_prev, uint64_t next, bool has_next, int K) {
    int best = 0;
    if (has_prev) best = key_common(prev, q, K);
    if (has_next) {
        const int c = key_common(next, q, K);
        best = c > best ? c : best;
    }
    return best < m ? best : m;
}

// Byte path: the symbols that the k-mer at p (sba bytes; a '$' ends it) shares with the sought one from
// the first on, at most m, in 4-bit codes: stops at the first difference or at code 0, and reads no
// byte after a '$'.
template <class Sought>
GKM_HD int bytes_match_len(const uint8_t *p, const uint8_t *lut4, const Sought &sought, int m) {
    int t = 0;
    for (; t < m; ++t) {
        const uint32_t x = lut4[p[t]];
        if (x == 0 || x != sought(t)) break;
    }
    return t;
}

// The insertion point of the sought m symbols among the k-mers at sba + starts[0, n) (ascending under
// bytes_cmp at every length up to the sort's): the number that compare below.
template <class Sought>
GKM_HD uint64_t bytes_lower_bound(const uint8_t *sba, const uint32_t *starts, uint64_t n, int m, const uint8_t *lut4,
                                  const Sought &sought) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (bytes_cmp<false>(sba + starts[mid], m, lut4, sought) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One position of the byte path: *len = the longest prefix of the sought m symbols that occurs,
// *first / *count = its range (0, 0 when *len is 0).
template <class Sought>
GKM_HD void bytes_match(const uint8_t *sba, const uint32_t *starts, uint64_t n, int m, const uint8_t *lut4,
                        const Sought &sought, uint32_t *len, uint64_t *first, uint32_t *count) {
    *len = 0;
    *first = 0;
    *count = 0;
    if (m <= 0 || n == 0) return;
    const uint64_t pos = bytes_lower_bound(sba, starts, n, m, lut4, sought);
    int l = 0;
    if (pos > 0) l = bytes_match_len(sba + starts[pos - 1], lut4, sought, m);
    if (pos < n) {
        const int c = bytes_match_len(sba + starts[pos], lut4, sought, m);
        l = c > l ? c : l;
    }
    if (l == 0) return;
    *len = (uint32_t)l;
    bytes_range<false>(sba, starts, n, l, lut4, sought, first, count);
}

// The per-sequence maximum as one word under a 64-bit max: the length above, below it the complement of
// the position's offset in its sequence, so that among equal lengths the first position wins whatever
// the order of the updates.  0 = nothing yet (a length of 0 is never recorded).
GKM_HD uint64_t best_pack(uint32_t len, uint32_t offset_in_seq) {
    return ((uint64_t)len << 32) | (uint64_t)(0xFFFFFFFFu - offset_in_seq);
}
GKM_HD uint32_t best_len(uint64_t w) { return (uint32_t)(w >> 32); }
GKM_HD uint32_t best_pos(uint64_t w) { return (w >> 32) ? 0xFFFFFFFFu - (uint32_t)w : 0u; }

}  // namespace match
}  // namespace gkm
