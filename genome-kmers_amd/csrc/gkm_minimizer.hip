// gkm_minimizer.hip -- gk_minimizers, gk_select_minimizers: minimizer sampling of a read batch or of the
// loaded sequence (gfx950).  The definition is include/gkm.h's; DESIGN.md §4, "Minimizers".
//
// One block owns a tile of kMzTile positions.  It stages the tile's bytes with a halo of w - 1 on the
// left and w - 1 + k - 1 on the right in LDS as 2-bit codes with a "not A/C/G/T" bit, marks the bytes
// at which a sequence of the batch starts (tile_seq_span, gkm_tile_seqs.h, then one pass over the
// offsets between its two ends: no table, so any number of sequence ends in a tile), rolls key and
// reverse complement per thread as screen_kernel does, and writes ord and a flag byte for the tile and
// its w - 1 neighbours on each side into LDS.  The windows are then decided by block-wise prefix / suffix minima
// (van Herk), O(log w) LDS steps per position whatever the ords; the equivalent local rule per position
// (minimizer::selected, gkm_minimizer_host.h) is what the driver under the host sanitizers checks.
// Ordered output without atomics: a count pass writes one count per tile, an exclusive scan over the
// chunk's tiles follows, and the emit pass -- the same kernel, deciding again instead of keeping a
// flag per position in memory -- places each selected position by ballot and popcount within its
// wave, the waves' counts summed in LDS.  So the result is ascending and the same on every run and for
// every chunk size.  per_seq follows from the sorted positions by two lower bounds per sequence.
#include <algorithm>
#include <cstring>

#include "gkm_internal.h"
#include "gkm_minimizer_host.h"
#include "gkm_screen_host.h"
#include "gkm_tile_seqs.h"

namespace gkm {

constexpr int kMzThreads = 256;
constexpr int kMzRounds = 4;  // positions per thread, position r * kMzThreads + tid in round r
constexpr int kMzTile = kMzThreads * kMzRounds;
constexpr int kMzWaves = kMzThreads / 64;
constexpr int kMzExt = kMzTile + 2 * ((int)minimizer::kMaxW - 1);  // ords: the tile and w - 1 on each side
constexpr int kMzCodes = kMzExt + (int)minimizer::kMaxK - 1;       // codes: the last ord's k-mer too

struct MzArgs {
    const uint8_t *bytes;        // bytes[i] is position held_lo + i
    uint64_t held_lo, held_hi;   // the positions whose bytes are here; any other reads as invalid
    uint64_t own_lo, own_hi;     // the positions this launch decides
    const uint64_t *offsets;     // [nseq + 1]; nseq == 0: one sequence (the loaded sba)
    uint64_t nseq, total;        // total: the batch's bytes (offsets[nseq])
    uint32_t k, w, flags;
    uint32_t *tile_count;        // count pass: [tiles]
    const uint32_t *tile_off;    // emit pass: their exclusive scan
    uint64_t out_base;           // emit pass: where the launch's first selected position goes
    uint64_t *pos, *key;         // emit pass of a batch
    uint8_t *strand;
    uint32_t *pos32;             // emit pass of the loaded sequence: the start set
};

template <bool EMIT>
__global__ __launch_bounds__(kMzThreads) void minimizer_kernel(const MzArgs a) {
    // per position: bits 0-1 the 2-bit code, bit 2 "not A/C/G/T"; s_start: 1 where a sequence starts (a plain
    // store of the same value by every thread that finds one: empty reads share an offset)
    __shared__ uint8_t s_code[kMzCodes];
    __shared__ uint8_t s_start[kMzCodes];
    __shared__ uint8_t s_flag[kMzExt];  // minimizer::kValid | kStrand | kSeqStart
    __shared__ uint64_t s_ord[kMzExt];
    __shared__ uint64_t s_key[kMzTile];
    __shared__ uint64_t s_j[2];
    __shared__ uint32_t s_cnt[kMzRounds * kMzWaves];
    const int tid = threadIdx.x, k = (int)a.k, w = (int)a.w;
    const uint64_t g0 = a.own_lo + blockIdx.x * (uint64_t)kMzTile;
    const uint64_t g1 = g0 + kMzTile < a.own_hi ? g0 + kMzTile : a.own_hi;
    const int own = (int)(g1 - g0);
    const int64_t e_lo = (int64_t)g0 - (w - 1);  // position of ord 0 (below 0 at the batch's start)
    const int E = own + 2 * (w - 1);             // ords: <= kMzExt
    const int ncodes = E + k - 1;                // codes: <= kMzCodes
    // the sequences of the first and last position staged that lie in the batch
    const uint64_t c_lo = e_lo < 0 ? 0 : (uint64_t)e_lo;
    const uint64_t c_hi = (uint64_t)(e_lo + ncodes) < a.total ? (uint64_t)(e_lo + ncodes) : a.total;
    if (a.nseq && tid < 64) tile_seq_span(a.offsets, a.nseq, c_lo, c_hi, tid, s_j);
    for (int i = tid; i < ncodes; i += kMzThreads) {
        const int64_t p = e_lo + i;
        uint8_t v = 4;  // outside the bytes held (only past an end of the batch): no valid start
        if (p >= (int64_t)a.held_lo && (uint64_t)p < a.held_hi) {
            const uint32_t b = a.bytes[(uint64_t)p - a.held_lo];
            const bool acgt = (b == 'A') | (b == 'C') | (b == 'G') | (b == 'T');
            v = acgt ? (uint8_t)canon_code<2>(b, nullptr) : (uint8_t)4;
        }
        s_code[i] = v;
        s_start[i] = 0;
    }
    __syncthreads();
    if (a.nseq) {  // the starts of the sequences after the first one's, all inside (c_lo, c_hi)
        const uint64_t j0 = s_j[0], j1 = s_j[1];
        for (uint64_t j = j0 + 1 + tid; j <= j1; j += kMzThreads) {
            const uint64_t o = a.offsets[j];
            if (o > c_lo && o < c_hi) s_start[(int64_t)o - e_lo] = 1;
        }
        __syncthreads();
    }
    // ords and flags of the E positions, a run of `per` consecutive ones per thread
    const bool canon = (a.flags & minimizer::kFlagCanonical) != 0, lex = (a.flags & minimizer::kFlagLex) != 0;
    const int per = (E + kMzThreads - 1) / kMzThreads;
    const int i0 = tid * per, i1 = i0 + per < E ? i0 + per : E;
    if (i0 < i1) {
        const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
        const int top = 2 * (k - 1);
        uint64_t key = 0, rck = 0;
        int clean = 0;  // A/C/G/T bytes of one sequence in a row up to the k-mer's last
        auto push = [&](int i) {
            const uint32_t c = s_code[i] | (s_start[i] ? 8u : 0u);
            key = ((key << 2) | (c & 3)) & mask;
            rck = (rck >> 2) | ((uint64_t)(3 - (c & 3)) << top);
            clean = (c & 4) ? 0 : (c & 8) ? 1 : clean + 1;
        };
        for (int t = 0; t < k; ++t) push(i0 + t);
        for (int e = i0;;) {
            uint32_t strand;
            const uint64_t ckey = minimizer::canonical_key(key, rck, canon, &strand);
            s_ord[e] = minimizer::ord_of(ckey, lex);
            s_flag[e] = (uint8_t)((clean >= k ? minimizer::kValid : 0) | (strand ? minimizer::kStrand : 0) |
                                  (s_start[e] ? minimizer::kSeqStart : 0));
            const int li = e - (w - 1);
            if (EMIT && li >= 0 && li < own) s_key[li] = ckey;  // (the count pass reads no key)
            if (++e >= i1) break;
            push(e + k - 1);
        }
    }
    __syncthreads();
    // the decision of the owned positions, position r * kMzThreads + tid in round r
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long m[kMzRounds];
    // Block-wise prefix / suffix minima (van Herk) over blocks of w ords, each built by a doubling scan in
    // LDS: s_p[i] / s_s[i] = the leftmost least ord of its block up to i / from i on, s_pb / s_sb = whether
    // that stretch holds an invalid start or a sequence start.  Window s .. s + w - 1 spans at most two
    // blocks: its minimizer is the better of s_s[s] and s_p[s + w - 1], ties to the left.  It exists iff no
    // start in it is invalid and no sequence starts after its first position.  (Against the direct L / R
    // scan of minimizer::selected: profiles/minimizer/ab_decision_method.txt.)
    constexpr int kPer = (kMzExt + kMzThreads - 1) / kMzThreads;
    __shared__ uint16_t s_p[kMzExt], s_s[kMzExt];
    __shared__ uint8_t s_pb[kMzExt], s_sb[kMzExt], s_sel[kMzExt];
    auto better = [&](int x, int y) {  // x lies left of y
        return s_ord[x] <= s_ord[y] ? x : y;
    };
    for (int i = tid; i < E; i += kMzThreads) {
        s_p[i] = s_s[i] = (uint16_t)i;
        s_pb[i] = s_sb[i] = (s_flag[i] & (minimizer::kValid | minimizer::kSeqStart)) == minimizer::kValid ? 0 : 1;
        s_sel[i] = 0;
    }
    __syncthreads();
    for (int d = 1; d < w; d <<= 1) {
        int np[kPer], ns[kPer];
        uint8_t npb[kPer], nsb[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = tid + j * kMzThreads;
            if (i >= E) break;
            const int b0 = i / w * w, b1 = b0 + w;  // the block of i
            np[j] = s_p[i], npb[j] = s_pb[i], ns[j] = s_s[i], nsb[j] = s_sb[i];
            if (i - d >= b0) np[j] = better(s_p[i - d], np[j]), npb[j] |= s_pb[i - d];
            if (i + d < b1 && i + d < E) ns[j] = better(ns[j], s_s[i + d]), nsb[j] |= s_sb[i + d];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = tid + j * kMzThreads;
            if (i >= E) break;
            s_p[i] = (uint16_t)np[j], s_pb[i] = npb[j], s_s[i] = (uint16_t)ns[j], s_sb[i] = nsb[j];
        }
        __syncthreads();
    }
    for (int s = tid; s + w <= E; s += kMzThreads) {
        const int e = s + w - 1;
        const bool aligned = s % w == 0;  // the window is one block: the suffix alone covers it
        // a sequence may start at s itself: s counts by its validity, the rest of its block by s_sb
        const bool bad = !(s_flag[s] & minimizer::kValid) || ((s + 1) % w != 0 && s + 1 < E && s_sb[s + 1]) ||
                         (!aligned && s_pb[e]);
        if (!bad) s_sel[better(s_s[s], s_p[e])] = 1;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kMzRounds; ++r) {
        const int li = r * kMzThreads + tid;
        const bool sel = li < own && s_sel[li + (w - 1)] != 0;
        m[r] = __ballot(sel);
        if (lane == 0) s_cnt[r * kMzWaves + wave] = (uint32_t)__popcll(m[r]);
    }
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) {
            uint32_t sum = 0;
            for (int i = 0; i < kMzRounds * kMzWaves; ++i) sum += s_cnt[i];
            a.tile_count[blockIdx.x] = sum;
        }
        return;
    }
    // ascending: rounds in order, waves in order, lanes in order
    const uint64_t base = a.out_base + a.tile_off[blockIdx.x];
    uint32_t before = 0;
#pragma unroll
    for (int r = 0; r < kMzRounds; ++r) {
        for (int wv = 0; wv < kMzWaves; ++wv) {
            if (wv == wave && ((m[r] >> lane) & 1)) {
                const uint64_t at = base + before + (uint32_t)__popcll(m[r] & ((1ull << lane) - 1));
                const int li = r * kMzThreads + tid;
                if (a.pos32) {
                    a.pos32[at] = (uint32_t)(g0 + li);
                } else {
                    a.pos[at] = g0 + li;
                    a.key[at] = s_key[li];
                    a.strand[at] = (s_flag[li + (w - 1)] & minimizer::kStrand) ? 1 : 0;
                }
            }
            before += s_cnt[r * kMzWaves + wv];
        }
    }
}

// per_seq[j] = the selected positions in [offsets[j], offsets[j + 1]): two lower bounds over pos
__global__ __launch_bounds__(256) void minimizer_per_seq_kernel(const uint64_t *__restrict__ pos, uint64_t n,
                                                                const uint64_t *__restrict__ offsets, uint64_t nseq,
                                                                uint32_t *__restrict__ per_seq) {
    const uint64_t j = blockIdx.x * (uint64_t)256 + threadIdx.x;
    if (j >= nseq) return;
    auto lower = [&](uint64_t v) {
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (pos[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    per_seq[j] = (uint32_t)(lower(offsets[j + 1]) - lower(offsets[j]));
}

namespace {

int check_params(gk_ctx *c, uint32_t k, uint32_t w, uint32_t flags) {
    if (k < 1 || k > minimizer::kMaxK) return fail(c, GK_E_ARG, "k must be in 1..32 (k = " + std::to_string(k) + ")");
    if (w < 1 || w > minimizer::kMaxW) return fail(c, GK_E_ARG, "w must be in 1..256 (w = " + std::to_string(w) + ")");
    if (flags & ~(GK_MINIMIZER_CANONICAL | GK_MINIMIZER_LEX))
        return fail(c, GK_E_ARG, "unknown flag bits (flags = " + std::to_string(flags) + ")");
    return GK_OK;
}

// the result buffers grown to `need` entries, the first c->mz_n kept
int mz_reserve(gk_ctx *c, uint64_t need, uint64_t hint) {
    if (need <= c->mz_cap && c->mz_pos) return GK_OK;
    const uint64_t cap = std::max<uint64_t>(std::max(need, hint), 1024);
    uint64_t *np = nullptr, *nk = nullptr;
    uint8_t *ns = nullptr;
    hipError_t e = dev_alloc(reinterpret_cast<void **>(&np), 8 * cap);
    if (e == hipSuccess) e = dev_alloc(reinterpret_cast<void **>(&nk), 8 * cap);
    if (e == hipSuccess) e = dev_alloc(reinterpret_cast<void **>(&ns), cap);
    if (e == hipSuccess && c->mz_n && c->mz_pos) {
        e = hipMemcpyAsync(np, c->mz_pos, 8 * c->mz_n, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nk, c->mz_key, 8 * c->mz_n, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ns, c->mz_strand, c->mz_n, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // the new buffers go, the old ones stay the context's
        for (void *p : {(void *)np, (void *)nk, (void *)ns})
            if (p) (void)dev_free(p);
        return hip_fail(c, e, "growing the minimizer view");
    }
    if (c->mz_pos) (void)dev_free(c->mz_pos);
    if (c->mz_key) (void)dev_free(c->mz_key);
    if (c->mz_strand) (void)dev_free(c->mz_strand);
    c->mz_pos = np;
    c->mz_key = nk;
    c->mz_strand = ns;
    c->mz_cap = cap;
    return GK_OK;
}

// the count pass over a.own_lo .. a.own_hi and the scan of its tiles: a.tile_off set, *m the selected
int count_pass(gk_ctx *c, MzArgs &a, uint32_t *d_cnt, uint32_t *d_off, uint64_t *m) {
    const uint64_t tiles = (a.own_hi - a.own_lo + kMzTile - 1) / kMzTile;
    a.tile_count = d_cnt;
    a.tile_off = d_off;
    int slot;
    timer_begin(c, "minimizer_count", &slot);
    timer_units(c, slot, a.own_hi - a.own_lo);
    hipLaunchKernelGGL(minimizer_kernel<false>, dim3((unsigned)tiles), dim3(kMzThreads), 0, c->stream, a);
    GK_TRY_HIP(c, hipGetLastError());
    timer_end(c, slot);
    GK_TRY_HIP(c, scan_u32_exclusive_pub(c, d_cnt, tiles, d_off, m));  // (synchronises the stream)
    return GK_OK;
}

int emit_pass(gk_ctx *c, const MzArgs &a) {
    const uint64_t tiles = (a.own_hi - a.own_lo + kMzTile - 1) / kMzTile;
    int slot;
    timer_begin(c, "minimizer_emit", &slot);
    timer_units(c, slot, a.own_hi - a.own_lo);
    hipLaunchKernelGGL(minimizer_kernel<true>, dim3((unsigned)tiles), dim3(kMzThreads), 0, c->stream, a);
    GK_TRY_HIP(c, hipGetLastError());
    timer_end(c, slot);
    return GK_OK;
}

}  // namespace
}  // namespace gkm

using namespace gkm;

extern "C" int gk_minimizers(gk_ctx *c, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t k,
                             uint32_t w, uint32_t flags, uint64_t *n_out, uint32_t *per_seq) {
    if (!c) return GK_E_ARG;
    if (!n_out) return fail(c, GK_E_ARG, "null n_out");
    if (int rc = check_params(c, k, w, flags)) return rc;
    if (nseq > 0) {
        if (!offsets) return fail(c, GK_E_ARG, "null offsets");
        uint64_t at = 0;
        switch (screen::validate_offsets(offsets, nseq, &at)) {  // (before any sequence byte is read)
            case screen::kOffsetsOk: break;
            case screen::kOffsetsStart: return fail(c, GK_E_ARG, "offsets[0] must be 0");
            case screen::kOffsetsDecrease:
                return fail(c, GK_E_ARG, "offsets decrease at sequence " + std::to_string(at));
            case screen::kOffsetsLong:
                return fail(c, GK_E_ARG, "sequence " + std::to_string(at) + " is longer than 2^32 - 1 bytes");
        }
    }
    const uint64_t total = nseq ? offsets[nseq] : 0;
    if (total && !seqs) return fail(c, GK_E_ARG, "null seqs");
    c->mz_valid = false;
    c->mz_n = 0;
    *n_out = 0;
    if (total == 0) {  // an empty view
        if (per_seq && nseq) std::memset(per_seq, 0, 4 * nseq);
        c->mz_valid = true;
        return GK_OK;
    }
    GK_TRY_HIP(c, hipSetDevice(c->device));
    const uint64_t step = minimizer::chunk_positions(opt("GKM_MINIMIZER_CHUNK"));
    const uint64_t nchunks = minimizer::chunk_count(total, step);
    const uint64_t cap_bytes = minimizer::chunk_bytes_max(total, step, k, w);
    const uint64_t cap_tiles = (std::min(step, total) + kMzTile - 1) / kMzTile;
    uint8_t *d_bytes;
    uint64_t *d_off;
    uint32_t *d_cnt, *d_toff;
    GK_TRY_HIP(c, scratch(c, "mz_bytes", cap_bytes, &d_bytes));
    GK_TRY_HIP(c, scratch(c, "mz_off", nseq + 1, &d_off));
    GK_TRY_HIP(c, scratch(c, "mz_cnt", cap_tiles, &d_cnt));
    GK_TRY_HIP(c, scratch(c, "mz_toff", cap_tiles, &d_toff));
    // one pinned slot (stage_reserve keeps two of the size it is given): every chunk's scan waits for the
    // stream, so the chunk's copy has been read before the host fills the slot again
    if (int rc = stage_reserve(c, ((cap_bytes + 1) / 2 + 255) / 256 * 256)) return rc;
    GK_TRY_HIP(c, hipMemcpyAsync(d_off, offsets, 8 * (nseq + 1), hipMemcpyHostToDevice, c->stream));

    MzArgs a{};
    a.bytes = d_bytes;
    a.offsets = d_off;
    a.nseq = nseq;
    a.total = total;
    a.k = k;
    a.w = w;
    a.flags = flags;
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
        uint64_t own_lo, own_n, held_lo, held_n;
        minimizer::chunk_range(total, step, k, w, ci, &own_lo, &own_n, &held_lo, &held_n);
        uint8_t *slot = c->stage_pin;  // (the host fills it while the emit pass of the chunk before runs)
        std::memcpy(slot, seqs + held_lo, held_n);
        GK_TRY_HIP(c, hipMemcpyAsync(d_bytes, slot, held_n, hipMemcpyHostToDevice, c->stream));
        a.held_lo = held_lo;
        a.held_hi = held_lo + held_n;
        a.own_lo = own_lo;
        a.own_hi = own_lo + own_n;
        uint64_t m = 0;
        if (int rc = count_pass(c, a, d_cnt, d_toff, &m)) return rc;
        if (m == 0) continue;
        // room for this chunk; beyond it, what the batch would need at the density seen so far
        const uint64_t seen = c->mz_n + m, done = own_lo + own_n;
        const uint64_t hint = (uint64_t)((double)seen * (double)total / (double)done * 1.1) + 1024;
        if (int rc = mz_reserve(c, seen, std::min(hint, total))) return rc;
        a.out_base = c->mz_n;
        a.pos = c->mz_pos;
        a.key = c->mz_key;
        a.strand = c->mz_strand;
        a.pos32 = nullptr;
        if (int rc = emit_pass(c, a)) return rc;
        c->mz_n = seen;
    }
    if (per_seq) {
        uint32_t *d_per;
        GK_TRY_HIP(c, scratch(c, "mz_per_seq", nseq, &d_per));
        hipLaunchKernelGGL(minimizer_per_seq_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, c->stream,
                           c->mz_pos, c->mz_n, d_off, nseq, d_per);
        GK_TRY_HIP(c, hipGetLastError());
        GK_TRY_HIP(c, hipMemcpyAsync(per_seq, d_per, 4 * nseq, hipMemcpyDeviceToHost, c->stream));
    }
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    *n_out = c->mz_n;
    c->mz_valid = true;
    return GK_OK;
}

extern "C" int gk_copy_minimizers(gk_ctx *c, uint64_t *pos, uint64_t *key, uint8_t *strand, uint64_t n) {
    if (!c) return GK_E_ARG;
    if (!c->mz_valid) return fail(c, GK_E_STATE, "no minimizer view: call gk_minimizers first");
    if (n != c->mz_n)
        return fail(c, GK_E_ARG, "n (" + std::to_string(n) + ") differs from the view's count (" + std::to_string(c->mz_n) + ")");
    if (n == 0) return GK_OK;
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (pos) GK_TRY_HIP(c, hipMemcpyAsync(pos, c->mz_pos, 8 * n, hipMemcpyDeviceToHost, c->stream));
    if (key) GK_TRY_HIP(c, hipMemcpyAsync(key, c->mz_key, 8 * n, hipMemcpyDeviceToHost, c->stream));
    if (strand) GK_TRY_HIP(c, hipMemcpyAsync(strand, c->mz_strand, n, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_device_minimizers(gk_ctx *c, void **pos, void **key, void **strand, uint64_t *n) {
    if (!c) return GK_E_ARG;
    if (!c->mz_valid) return fail(c, GK_E_STATE, "no minimizer view: call gk_minimizers first");
    if (pos) *pos = c->mz_pos;
    if (key) *key = c->mz_key;
    if (strand) *strand = c->mz_strand;
    if (n) *n = c->mz_n;
    return GK_OK;
}

extern "C" int gk_select_minimizers(gk_ctx *c, uint32_t k, uint32_t w, uint32_t flags, uint64_t *n_out) {
    if (!c) return GK_E_ARG;
    if (int rc = check_params(c, k, w, flags)) return rc;
    if (!c->sba || c->sba_len == 0) return fail(c, GK_E_STATE, "no sequence loaded");
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive; a refused call has touched nothing)
    GK_TRY_HIP(c, hipSetDevice(c->device));
    const uint64_t L = c->sba_len;
    const uint64_t tiles = (L + kMzTile - 1) / kMzTile;
    uint32_t *d_cnt, *d_toff;
    GK_TRY_HIP(c, scratch(c, "mz_cnt", tiles, &d_cnt));
    GK_TRY_HIP(c, scratch(c, "mz_toff", tiles, &d_toff));
    MzArgs a{};
    a.bytes = c->sba;
    a.held_lo = 0;
    a.held_hi = L;
    a.own_lo = 0;
    a.own_hi = L;
    a.total = L;
    a.k = k;
    a.w = w;
    a.flags = flags;
    uint64_t n = 0;
    if (int rc = count_pass(c, a, d_cnt, d_toff, &n)) return rc;
    c->have_starts = false;  // (ensure_elems keeps no starts of the earlier set)
    if (int rc = ensure_elems(c, std::max<uint64_t>(n, 1), 1)) return rc;
    c->cur = 0;
    if (n) {
        a.out_base = 0;
        a.pos32 = c->vals[0];
        if (int rc = emit_pass(c, a)) return rc;
    }
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    c->min_k = k;
    set_kmer_set(c, KmerSet::Given);
    if (n_out) *n_out = n;
    return GK_OK;
}
