// gkm_mismatch_host.h -- the host-only pieces of gk_lookup_mismatch (gkm_mismatch.hip): the reverse
// complement of a query, its 2-bit word and its 4-bit words, chunk arithmetic, and the sort and split
// of the hit records.  Plain C++ (no HIP), so that a stand-alone driver can run them under the host
// sanitizers (tests/sanitize/mismatch_driver.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>

#include "gkm_canon.h"
#include "gkm_lookup_host.h"

namespace gkm {
namespace mismatch {

constexpr uint32_t kMaxQlen = 32;  // one 64-bit word of 2-bit codes, two of 4-bit codes

// queries per launch (each launch is one pass over the k-mers): bounds the per-chunk device state,
// 16 bytes of query words per comparison and 8 (max_mismatches + 1) bytes of counts per query, at
// under 20 MiB; GKM_MISMATCH_CHUNK can lower it (chunk_size)
constexpr uint64_t kChunk = 1ull << 16;

inline uint64_t chunk_size(const char *value) { return query::knob_below(value, kChunk); }
using lookup::chunk_count;
using lookup::chunk_range;

// dst = reverse complement of q (the reference's IUPAC complement, lookup::complement); dst != q
inline void reverse_complement(const uint8_t *q, uint32_t qlen, uint8_t *dst) {
    for (uint32_t j = 0; j < qlen; ++j) dst[j] = lookup::complement(q[qlen - 1 - j]);
}

// A C G T -> 0 1 2 3 (gkm_canon.h canon_code<2>)
inline uint32_t code2(uint8_t b) { return ((b >> 1) ^ (b >> 2)) & 3u; }
// '$' and anything else 0, A B C D G H K M N R S T V W Y -> 1..15: the kernels' own
using gkm::code4;

// the 2 qlen-bit prefix word of an A/C/G/T query, first base most significant, right-aligned (as
// lookup_keys_kernel builds it): qlen <= 32, no shift by 64 and no mask at qlen = 32
inline uint64_t encode2(const uint8_t *q, uint32_t qlen) {
    uint64_t w = 0;
    for (uint32_t t = 0; t < qlen; ++t) w = (w << 2) | code2(q[t]);
    return w;
}

// the two words of 4-bit codes of a query: symbol t in bits [4 (t % 16), 4 (t % 16) + 4) of word
// t / 16; the nibbles from qlen on are 0 (qlen <= 32)
inline void encode4(const uint8_t *q, uint32_t qlen, uint64_t out[2]) {
    out[0] = out[1] = 0;
    for (uint32_t t = 0; t < qlen; ++t) out[t >> 4] |= (uint64_t)code4(q[t]) << (4 * (t & 15));
}

// one hit as the kernel appends it, in no particular order
struct HitRecord {
    uint64_t kmer_num;     // position in the current start-index order
    uint32_t query;        // index in the caller's batch
    uint16_t mismatches;
    uint16_t strand;       // 0: the query as given, 1: its reverse complement
};
static_assert(sizeof(HitRecord) == 16, "the kernel writes 16-byte records");

inline bool hit_less(const HitRecord &a, const HitRecord &b) {
    if (a.query != b.query) return a.query < b.query;
    if (a.kmer_num != b.kmer_num) return a.kmer_num < b.kmer_num;
    return a.strand < b.strand;
}

// the records in ascending (query, kmer_num, strand), split into the caller's four arrays
inline void sort_and_split(HitRecord *rec, uint64_t n, uint32_t *hit_query, uint64_t *hit_kmer_num,
                           uint8_t *hit_mismatches, uint8_t *hit_strand) {
    std::sort(rec, rec + n, hit_less);
    for (uint64_t i = 0; i < n; ++i) {
        hit_query[i] = rec[i].query;
        hit_kmer_num[i] = rec[i].kmer_num;
        hit_mismatches[i] = (uint8_t)rec[i].mismatches;
        hit_strand[i] = (uint8_t)rec[i].strand;
    }
}

}  // namespace mismatch
}  // namespace gkm
