// gkm_lookup_host.h -- the host-only pieces of gk_lookup (gkm_lookup.hip): query validation, the
// canonical form of a query, chunk arithmetic.  Plain C++ (no HIP), so that a stand-alone driver can
// run them under the host sanitizers (tests/sanitize/lookup_driver.cpp).
#pragma once

#include <stdint.h>

#include <cstring>

#include "gkm_query_host.h"

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace gkm {
namespace lookup {

// queries per launch: bounds the device scratch and the pinned staging (chunk * (qlen + 12) bytes,
// the staging twice); GKM_LOOKUP_CHUNK can lower it (chunk_size)
constexpr uint64_t kChunk = 1ull << 20;

// 1: A C G T, 2: the other sba letters (B D H K M N R S V W Y), 0: anything else ('$' included)
inline int query_class(uint8_t b) {
    switch (b) {
        case 'A': case 'C': case 'G': case 'T': return 1;
        case 'B': case 'D': case 'H': case 'K': case 'M': case 'N': case 'R': case 'S': case 'V': case 'W':
        case 'Y': return 2;
        default: return 0;
    }
}

// every byte of p[0, len) is A, C, G or T (AVX2 where the CPU has it: four compares per 32 bytes, as
// the packed transfer's alphabet check, gkm_xfer.hip)
inline bool block_is_acgt_scalar(const uint8_t *p, uint64_t len) {
    unsigned bad = 0;
    for (uint64_t i = 0; i < len; ++i) {
        const uint8_t b = p[i];
        bad |= !((b == 'A') | (b == 'C') | (b == 'G') | (b == 'T'));
    }
    return bad == 0;
}
#if defined(__x86_64__)
__attribute__((target("avx2"))) inline bool block_is_acgt_avx2(const uint8_t *p, uint64_t len) {
    const __m256i cA = _mm256_set1_epi8('A'), cC = _mm256_set1_epi8('C'), cG = _mm256_set1_epi8('G'),
                  cT = _mm256_set1_epi8('T');
    __m256i all = _mm256_set1_epi8((char)0xFF);
    uint64_t i = 0;
    for (; i + 32 <= len; i += 32) {
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i));
        const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, cA), _mm256_cmpeq_epi8(v, cC)),
                                           _mm256_or_si256(_mm256_cmpeq_epi8(v, cG), _mm256_cmpeq_epi8(v, cT)));
        all = _mm256_and_si256(all, ok);
    }
    if ((uint32_t)_mm256_movemask_epi8(all) != 0xFFFFFFFFu) return false;
    return block_is_acgt_scalar(p + i, len - i);
}
#endif
inline bool block_is_acgt(const uint8_t *p, uint64_t len) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return block_is_acgt_avx2(p, len);
#endif
    return block_is_acgt_scalar(p, len);
}

// index (into the m * qlen bytes) of the first byte outside the alphabet, or -1; *all_acgt: every
// byte is A, C, G or T
inline int64_t validate_queries(const uint8_t *q, uint64_t m, uint32_t qlen, bool *all_acgt) {
    bool acgt = true;
    const uint64_t total = m * (uint64_t)qlen;
    // The check is on the call's critical path (a 1e7 x 31 batch is 310 MB), so the common case, a
    // block of A/C/G/T only, is four byte compares in a loop the compiler vectorises; only a block
    // that fails it is classified byte by byte.
    constexpr uint64_t kBlock = 4096;
    for (uint64_t at = 0; at < total; at += kBlock) {
        const uint64_t len = total - at < kBlock ? total - at : kBlock;
        const uint8_t *p = q + at;
        if (block_is_acgt(p, len)) continue;
        acgt = false;
        for (uint64_t i = 0; i < len; ++i)
            if (query_class(p[i]) == 0) {
                *all_acgt = false;
                return (int64_t)(at + i);
            }
    }
    *all_acgt = acgt;
    return -1;
}

// the reference's IUPAC complement (sequence_collection.py:402-433; gkm_canon.h kComp4 on codes)
inline uint8_t complement(uint8_t b) {
    switch (b) {
        case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'R': return 'Y'; case 'Y': return 'R'; case 'K': return 'M'; case 'M': return 'K';
        case 'B': return 'V'; case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D';
        default: return b;  // S W N
    }
}

// dst = min(q, reverse complement of q) in the reference's byte order (dst != q)
inline void canonical_query(const uint8_t *q, uint32_t qlen, uint8_t *dst) {
    bool rc = false;
    for (uint32_t j = 0; j < qlen; ++j) {
        const uint8_t f = q[j], r = complement(q[qlen - 1 - j]);
        if (f != r) {
            rc = r < f;
            break;
        }
    }
    if (!rc) {
        std::memcpy(dst, q, qlen);
        return;
    }
    for (uint32_t j = 0; j < qlen; ++j) dst[j] = complement(q[qlen - 1 - j]);
}

// queries per launch: kChunk, cut so that a chunk's query bytes stay within kChunkBytes for long
// queries; the knob only lowers it (query::knob_below)
constexpr uint64_t kChunkBytes = 64ull << 20;
inline uint64_t chunk_size(const char *value, uint32_t qlen) {
    const uint64_t fit = kChunkBytes / qlen ? kChunkBytes / qlen : 1;
    return query::knob_below(value, kChunk < fit ? kChunk : fit);
}

inline uint64_t chunk_count(uint64_t m, uint64_t chunk) { return m / chunk + (m % chunk != 0); }

// [*off, *off + *len) of chunk i
inline void chunk_range(uint64_t m, uint64_t chunk, uint64_t i, uint64_t *off, uint64_t *len) {
    *off = i * chunk;
    *len = m - *off < chunk ? m - *off : chunk;
}

}  // namespace lookup
}  // namespace gkm
