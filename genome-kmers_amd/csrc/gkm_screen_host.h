// gkm_screen_host.h -- the host-only pieces of gk_screen (gkm_screen.hip): offset validation, the
// chunk and overlap arithmetic, mapping a byte position back to (sequence, offset), the knobs' values.
// Plain C++ (no HIP), so that a stand-alone driver can run them under the host sanitizers
// (tests/sanitize/screen_driver.cpp).
#pragma once

#include <stdint.h>

#include "gkm_query_host.h"

namespace gkm {
namespace screen {

// bytes of reads per launch, the K - 1 bytes a chunk shares with the next one included: bounds the
// device scratch (5 B per byte with per-window counts) and the pinned staging (the same, twice);
// GKM_SCREEN_CHUNK can lower it (chunk_bytes)
constexpr uint64_t kChunkBytes = 16ull << 20;

enum OffsetError { kOffsetsOk = 0, kOffsetsStart = 1, kOffsetsDecrease = 2, kOffsetsLong = 3 };

// offsets[0 .. nseq]: starts at 0, never decreases, no sequence over 2^32 - 1 bytes.  *at: the
// sequence that breaks the rule.  Reads the offsets only, never a sequence byte.
inline OffsetError validate_offsets(const uint64_t *offsets, uint64_t nseq, uint64_t *at) {
    *at = 0;
    if (offsets[0] != 0) return kOffsetsStart;
    for (uint64_t j = 0; j < nseq; ++j) {
        *at = j;
        if (offsets[j + 1] < offsets[j]) return kOffsetsDecrease;
        if (offsets[j + 1] - offsets[j] > 0xFFFFFFFFull) return kOffsetsLong;
    }
    return kOffsetsOk;
}

using query::parse_path;  // GKM_SCREEN_PATH

// bytes per launch for windows of K bytes: kChunkBytes, lowered by the knob (query::knob_below), and
// at least K so that a chunk holds one whole window
inline uint64_t chunk_bytes(const char *value, uint32_t K) {
    const uint64_t c = query::knob_below(value, kChunkBytes);
    return c < K ? (uint64_t)K : c;
}

// A chunk of `chunk` >= K bytes owns the positions [start, start + nslots): it checks their bytes and
// answers the windows that start there, and holds the bytes [start, start + nbytes), K - 1 more than
// it owns (fewer at the batch's end), so that every window it answers lies inside it.  Consecutive
// chunks are chunk - (K - 1) positions apart: every position of [0, total) is owned exactly once.
inline uint64_t chunk_step(uint64_t chunk, uint32_t K) { return chunk - (K - 1); }
inline uint64_t chunk_count(uint64_t total, uint64_t chunk, uint32_t K) {
    const uint64_t step = chunk_step(chunk, K);
    return total / step + (total % step != 0);
}
inline void chunk_range(uint64_t total, uint64_t chunk, uint32_t K, uint64_t i, uint64_t *start, uint64_t *nslots,
                        uint64_t *nbytes) {
    const uint64_t step = chunk_step(chunk, K);
    *start = i * step;
    const uint64_t left = total - *start;
    *nslots = left < step ? left : step;
    *nbytes = left < chunk ? left : chunk;
}

// the sequence that holds byte position pos < offsets[nseq] (the last j with offsets[j] <= pos: empty
// sequences at pos are passed over) and the position's offset in it
inline void locate(const uint64_t *offsets, uint64_t nseq, uint64_t pos, uint64_t *seq, uint64_t *off) {
    uint64_t lo = 0, hi = nseq;  // first u in [0, nseq] with offsets[u] > pos
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    *seq = lo - 1;
    *off = pos - offsets[lo - 1];
}

}  // namespace screen
}  // namespace gkm
