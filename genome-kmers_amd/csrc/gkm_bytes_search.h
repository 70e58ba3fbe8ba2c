// gkm_bytes_search.h -- the byte path of gk_lookup, gk_join and gk_screen: one comparison of a k-mer
// of the sba with a sought k-mer in 4-bit symbol codes, and the range search over the sorted starts
// built on it.  Plain C++ (GKM_HD, gkm_canon.h), so the kernels and a stand-alone driver under the
// host sanitizers (tests/sanitize/bytes_search_driver.cpp) run the same code.
//
// The callers differ only in where symbol t of the sought k-mer comes from: a Sought is a small
// struct whose operator()(int t) gives its 4-bit code.
#pragma once

#include "gkm_canon.h"

namespace gkm {

// gk_lookup: the thread's column of the block's LDS copy of the queries' codes, [qlen][256] ...
struct SoughtLds {
    const uint8_t *col;
    GKM_HD uint32_t operator()(int t) const { return col[t * 256]; }
};
// ... or the query bytes where they lie
struct SoughtBytes {
    const uint8_t *q, *lut4;
    GKM_HD uint32_t operator()(int t) const { return lut4[q[t]]; }
};
// The k bytes at q, or their reverse complement when rc.  gk_join: A's k-mer at its group head in A's
// sba, rc = canon_is_rc of it on canonical orders (found once, outside the search), false on forward
// ones; gk_screen: the read's window in place, rc = the strand that is sought.
struct SoughtStrand {
    const uint8_t *q, *lut4;
    int k;
    bool rc;
    GKM_HD uint32_t operator()(int t) const { return canon_sym<4>(q, k, t, rc, lut4); }
};

// sign of (the k-mer at p, its canonical form if CANON) - (sought) over k symbols in 4-bit codes
// through lut4.  An equal pair of code 0 ends the comparison as equal.  This one form serves every
// caller: gk_lookup's queries are checked on the host and gk_join's sides hold whole k-mers only, so
// their sought codes are never 0 and a '$' in the k-mer compares below and ends the loop there; in
// gk_screen a byte outside the alphabet that has not failed the call yet (code 0) can meet the '$'.
// Either way no byte after the '$' that ends a contig is read (canonical orders hold whole k-mers
// only: p[0, k) has no '$').
template <bool CANON, class Sought>
GKM_HD int bytes_cmp(const uint8_t *__restrict__ p, int k, const uint8_t *lut4, const Sought &sought) {
    const bool rc = CANON && canon_is_rc<4>(p, k, lut4);
    uint32_t x = 0, y = 0;
    for (int t = 0; t < k; ++t) {  // (one exit test per symbol; the sign is taken once, after the loop)
        x = CANON ? canon_sym<4>(p, k, t, rc, lut4) : (uint32_t)lut4[p[t]];
        y = sought(t);
        if (x != y || x == 0) break;
    }
    return x < y ? -1 : (int)(x > y);
}

// The k-mers at sba + starts[0, n) ascend under bytes_cmp: *first = the number below the sought
// k-mer, *count = the number equal to it (the lower bound, then the upper bound from it on).
template <bool CANON, class Sought>
GKM_HD void bytes_range(const uint8_t *__restrict__ sba, const uint32_t *__restrict__ starts, uint64_t n, int k,
                        const uint8_t *lut4, const Sought &sought, uint64_t *first, uint32_t *count) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {  // k-mers below the sought one
        const uint64_t mid = (lo + hi) >> 1;
        if (bytes_cmp<CANON>(sba + starts[mid], k, lut4, sought) < 0) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t lb = lo;
    hi = n;
    while (lo < hi) {  // ... and not above it, from the lower bound on
        const uint64_t mid = (lo + hi) >> 1;
        if (bytes_cmp<CANON>(sba + starts[mid], k, lut4, sought) <= 0) lo = mid + 1;
        else hi = mid;
    }
    *first = lb;
    *count = (uint32_t)(lo - lb);
}

}  // namespace gkm
