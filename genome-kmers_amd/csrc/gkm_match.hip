// gkm_match.hip -- gk_match: matching statistics of a batch of reads against the sorted index (gfx950).
//
// For every byte position p of every sequence of the batch: the length of the longest prefix of the
// bytes from p on (inside the sequence, at most the cap C) that gk_lookup finds in the index, and that
// prefix's range of sorted positions; per sequence the longest such length, the first position that
// attains it and the sum of the lengths ("Matching statistics").  The sorted order is a
// prefix-sorted list, so the longest prefix is attained next to the insertion point of the bytes: one
// lower-bound search, a comparison with the two neighbours (gkm_match_host.h), one range search at the
// length found.  The batch crosses the link once, in chunks that overlap by C - 1 bytes (gk_screen's
// chunking with C in the place of K).  Two paths, the same answers:
//   keys   final one-word 2-bit keys in sorted order (lookup_keys_usable): a block stages a tile of
//          positions plus a C - 1 halo in LDS as 2-bit codes and flags; a thread builds, per position,
//          the key of its m symbols -- cut at the sequence's end, the cap and the first letter other
//          than A, C, G, T, which the index does not hold -- followed by zeros, and its positions'
//          searches advance in lockstep (key_lower_bound, key_search_each: gkm_lookup_search.h).
//   bytes  one search per position over the sorted starts, comparing sba bytes with the read's in 4-bit
//          codes where they lie (bytes_match, gkm_match_host.h over gkm_bytes_search.h).  Always valid.
// The tile's sequences are found and walked as in gk_screen (gkm_tile_seqs.h); per sequence a block
// adds the lengths in LDS and keeps the maximum as one packed word (match::best_pack), then issues one
// global atomic per (block, sequence) and counter.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gkm_internal.h"
#include "gkm_lookup_search.h"
#include "gkm_match_host.h"
#include "gkm_tile_seqs.h"

#ifndef GKM_MATCH_WIN
// positions per thread: gk_screen's value (profiles/screen/ab_windows_per_thread.txt); no A/B of its
// own has been run
#define GKM_MATCH_WIN 4
#endif

namespace gkm {

constexpr int kMatchThreads = 256;
constexpr int kMatchWin = GKM_MATCH_WIN;
constexpr int kMatchTile = kMatchThreads * kMatchWin;  // positions per block
constexpr int kMatchBounds = 256;                      // sequence ends a pass keeps in LDS
constexpr int kMatchHalo = 31;                         // key path: C <= K <= 32

struct MatchArgs {
    const uint8_t *bytes;     // the chunk: bytes [base, base + nbytes) of the batch
    uint64_t base, nslots, nbytes;  // the chunk owns the positions [base, base + nslots)
    const uint64_t *offsets;  // [nseq + 1]
    uint64_t nseq;
    uint32_t K, C;            // the sort length (key path), the cap
    const uint64_t *keys;     // key path
    const uint32_t *dir;
    int D;
    const uint8_t *sba;       // byte path
    const uint32_t *starts;
    uint64_t n;
    unsigned long long *sum;   // [nseq]
    unsigned long long *best;  // [nseq] match::best_pack words
    uint32_t *mlen;            // [nslots] each, or null
    unsigned long long *mfirst;
    uint32_t *mcount;
    unsigned long long *bad;   // smallest position of a byte outside the alphabet
};

// KEYS: the key path, else the byte path.  One block per tile of kMatchTile positions.
template <bool KEYS>
__global__ __launch_bounds__(kMatchThreads) void match_kernel(const MatchArgs a) {
    constexpr int W = kMatchWin;
    __shared__ uint8_t s_lut4[256];
    // key path: per position, bits 0-1 the 2-bit code, bit 2 "not A/C/G/T"
    __shared__ uint8_t s_code[KEYS ? kMatchTile + kMatchHalo : 1];
    __shared__ uint64_t s_tab[kMatchBounds];  // ends of the pass's sequences
    __shared__ unsigned long long s_sum[kMatchBounds];
    __shared__ unsigned long long s_best[kMatchBounds];
    __shared__ uint64_t s_j[2];
    const int tid = threadIdx.x;
    const int K = (int)a.K, C = (int)a.C;
    s_lut4[tid] = code4(tid);
    const uint64_t t0 = blockIdx.x * (uint64_t)kMatchTile;  // in the chunk
    const uint64_t t1 = t0 + kMatchTile < a.nslots ? t0 + kMatchTile : a.nslots;
    const uint64_t g0 = a.base + t0, g1 = a.base + t1;      // in the batch
    if (tid < 64) tile_seq_span(a.offsets, a.nseq, g0, g1, tid, s_j);  // the tile's first and last sequence
    __syncthreads();
    // the alphabet check of the positions the tile owns; the key path's staging with its halo
    if (KEYS) {
        const uint64_t have = a.nbytes - t0;
        for (int i = tid; i < kMatchTile + C - 1; i += kMatchThreads) {
            uint8_t v = 4;  // past the chunk: no match that counts reaches here
            if ((uint64_t)i < have) {
                const uint32_t b = a.bytes[t0 + i];
                const bool acgt = (b == 'A') | (b == 'C') | (b == 'G') | (b == 'T');
                v = acgt ? (uint8_t)canon_code<2>(b, nullptr) : (uint8_t)4;
                if ((uint64_t)i < t1 - t0 && s_lut4[b] == 0) atomicMin(a.bad, (unsigned long long)(g0 + i));
            }
            s_code[i] = v;
        }
    } else {
        for (int i = tid; (uint64_t)i < t1 - t0; i += kMatchThreads)
            if (s_lut4[a.bytes[t0 + i]] == 0) atomicMin(a.bad, (unsigned long long)(g0 + i));
    }
    const uint64_t j0 = s_j[0], j1 = s_j[1];
    const uint64_t pt0 = g0 + (uint64_t)tid * W;  // this thread's run of positions
    const uint64_t pt1 = pt0 + W < g1 ? pt0 + W : g1;
    auto init = [&](int i) {
        s_sum[i] = 0;
        s_best[i] = 0;
    };
    auto body = [&](uint64_t ja, int cnt, uint64_t slab_lo, uint64_t slab_hi) {
        const uint64_t pa = slab_lo > pt0 ? slab_lo : pt0, pb = slab_hi < pt1 ? slab_hi : pt1;
        if (pa >= pb) return;
        int jr = pass_seq_of(s_tab, cnt, pa);  // the sequence of pa in the pass
        const uint64_t first_start = a.offsets[ja];  // where the pass's first sequence starts
        const int np = (int)(pb - pa);
        int cur = jr;
        unsigned long long sum = 0, best = 0;
        auto flush = [&]() {
            if (sum) atomicAdd(&s_sum[cur], sum);
            if (best) atomicMax(&s_best[cur], best);
        };
        // position p of sequence jr (in the pass) matched len symbols
        auto record = [&](uint64_t p, int jr_p, uint32_t len, uint64_t first, uint32_t count) {
            const uint64_t slot = p - a.base;
            if (a.mlen) a.mlen[slot] = len;
            if (a.mfirst) a.mfirst[slot] = first;
            if (a.mcount) a.mcount[slot] = count;
            if (jr_p != cur) {
                flush();
                cur = jr_p;
                sum = 0;
                best = 0;
            }
            if (len) {
                const uint64_t seq_start = jr_p == 0 ? first_start : s_tab[jr_p - 1];
                const unsigned long long wd = match::best_pack(len, (uint32_t)(p - seq_start));
                sum += len;
                best = wd > best ? wd : best;
            }
        };
        if (KEYS) {
            const int li = (int)(pa - g0);
            uint64_t q[W], pos[W], prefix[W], f[W];
            uint32_t cn[W];
            int ms[W], ls[W], sj[W];
            bool act[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                q[w] = 0;
                ms[w] = 0;
                sj[w] = 0;
                act[w] = false;
                if (w >= np) continue;
                const uint64_t p = pa + w;
                while (s_tab[jr] <= p) ++jr;
                sj[w] = jr;
                const uint64_t room = s_tab[jr] - p;  // bytes to the sequence's end
                const int lim = room < (uint64_t)C ? (int)room : C;
                uint64_t key = 0;
                int m = 0;
                for (; m < lim; ++m) {  // the clean symbols from p on
                    const uint32_t c = s_code[li + w + m];
                    if (c & 4) break;
                    key = (key << 2) | c;
                }
                ms[w] = m;
                q[w] = m ? key << (2 * (K - m)) : 0;  // (m >= 1: a shift of at most 62)
                act[w] = m > 0;
            }
            key_lower_bound<W>(a.keys, a.n, a.dir, a.D, 2 * K, q, act, pos);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                ls[w] = 0;
                prefix[w] = 0;
                if (act[w]) {
                    const bool has_prev = pos[w] > 0, has_next = pos[w] < a.n;
                    const uint64_t prev = has_prev ? a.keys[pos[w] - 1] : 0, next = has_next ? a.keys[pos[w]] : 0;
                    ls[w] = match::key_match_len(q[w], ms[w], prev, has_prev, next, has_next, K);
                }
                act[w] = ls[w] > 0;
                if (act[w]) prefix[w] = q[w] >> (2 * (K - ls[w]));
            }
            key_search_each<W>(a.keys, a.n, a.dir, a.D, 2 * K, ls, prefix, act, f, cn);
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < np) record(pa + w, sj[w], (uint32_t)ls[w], f[w], cn[w]);
        } else {
            for (uint64_t p = pa; p < pb; ++p) {
                while (s_tab[jr] <= p) ++jr;
                const uint64_t room = s_tab[jr] - p;
                const int m = room < (uint64_t)C ? (int)room : C;
                uint32_t len, count;
                uint64_t first;
                match::bytes_match(a.sba, a.starts, a.n, m, s_lut4, SoughtBytes{a.bytes + (p - a.base), s_lut4}, &len,
                                   &first, &count);
                record(p, jr, len, first, count);
            }
        }
        flush();
    };
    auto flush_seq = [&](int i, uint64_t j) {
        if (s_sum[i]) atomicAdd(&a.sum[j], s_sum[i]);
        if (s_best[i]) atomicMax(&a.best[j], s_best[i]);
    };
    tile_seq_passes<kMatchBounds, kMatchThreads>(a.offsets, j0, j1, g0, g1, s_tab, tid, init, body, flush_seq);
}

}  // namespace gkm

using namespace gkm;

extern "C" int gk_match(gk_ctx *c, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t max_len,
                        uint32_t flags, uint32_t *longest, uint32_t *longest_pos, uint64_t *sum_len,
                        uint32_t *match_len, uint64_t *match_first, uint32_t *match_count) {
    if (!c) return GK_E_ARG;
    if (nseq == 0) return GK_OK;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sba) return fail(c, GK_E_STATE, "gk_match: no sequence loaded");
    if (!c->have_starts || !c->sorted)
        return fail(c, GK_E_STATE, "gk_match: the k-mers are not sorted: call gk_sort first");
    if (c->canonical)
        return fail(c, GK_E_UNSUPPORTED, "canonical k-mers have no prefixes: gk_match needs a forward order");
    if (!offsets || !longest || !longest_pos || !sum_len) return fail(c, GK_E_ARG, "gk_match: null array");
    if (flags != 0) return fail(c, GK_E_ARG, "gk_match: flags (" + std::to_string(flags) + ") must be 0");
    const uint32_t C = match::resolve_cap(c->sort_len, max_len);
    if (C == 0) {
        if (c->sort_len != 0)
            return fail(c, GK_E_ARG, "gk_match: max_len (" + std::to_string(max_len) + ") is above the sort length (" +
                                         std::to_string(c->sort_len) + ")");
        return fail(c, GK_E_ARG, "gk_match: max_len (" + std::to_string(max_len) + ") must be in 1.." +
                                     std::to_string(match::kMaxCap) + " after a sort with max_kmer_len None");
    }
    uint64_t at = 0;
    switch (screen::validate_offsets(offsets, nseq, &at)) {  // (before any sequence byte is read)
        case screen::kOffsetsOk: break;
        case screen::kOffsetsStart: return fail(c, GK_E_ARG, "offsets[0] must be 0");
        case screen::kOffsetsDecrease:
            return fail(c, GK_E_ARG, "offsets decrease at sequence " + std::to_string(at));
        case screen::kOffsetsLong:
            return fail(c, GK_E_ARG, "sequence " + std::to_string(at) + " is longer than 2^32 - 1 bytes");
    }
    const uint64_t total = offsets[nseq];
    if (total == 0) {
        std::memset(longest, 0, 4 * nseq);
        std::memset(longest_pos, 0, 4 * nseq);
        std::memset(sum_len, 0, 8 * nseq);
        return GK_OK;
    }
    if (!seqs) return fail(c, GK_E_ARG, "gk_match: null array");
    // path: the keys when the context holds final 2-bit keys (an A/C/G/T-only index: a match ends at any
    // other letter there), else the bytes
    const bool keys_ok = lookup_keys_usable(c);
    bool use_keys = keys_ok;
    const int path = query::parse_path(opt("GKM_MATCH_PATH"));
    if (path < 0) return fail(c, GK_E_ARG, "GKM_MATCH_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !keys_ok)
        return fail(c, GK_E_UNSUPPORTED, "GKM_MATCH_PATH=keys: the context holds no final one-word 2-bit forward keys");
    if (path == query::kPathBytes) use_keys = false;
    const char *dir_opt = opt("GKM_LOOKUP_DIR");
    const bool use_dir = !(dir_opt && std::strcmp(dir_opt, "0") == 0);
    const uint64_t chunk = match::chunk_bytes(opt("GKM_MATCH_CHUNK"), C);
    const uint64_t step = screen::chunk_step(chunk, C);

    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (int rc = materialize_starts(c)) return rc;
    uint32_t *dir = nullptr;
    if (use_keys && use_dir)
        if (int rc = lookup_build_dir(c, &dir)) return rc;

    const uint64_t cap_bytes = std::min(chunk, total), cap_slots = std::min(step, total);
    uint8_t *d_bytes;
    uint64_t *d_off;
    uint32_t *d_len = nullptr, *d_count = nullptr;
    unsigned long long *d_sum, *d_best, *d_bad, *d_first = nullptr;
    GK_TRY_HIP(c, scratch(c, "match_bytes", cap_bytes, &d_bytes));
    GK_TRY_HIP(c, scratch(c, "match_off", nseq + 1, &d_off));
    GK_TRY_HIP(c, scratch(c, "match_sum", nseq, &d_sum));
    GK_TRY_HIP(c, scratch(c, "match_best", nseq, &d_best));
    GK_TRY_HIP(c, scratch(c, "match_bad", 1, &d_bad));
    if (match_len) GK_TRY_HIP(c, scratch(c, "match_len", cap_slots, &d_len));
    if (match_first) GK_TRY_HIP(c, scratch(c, "match_first", cap_slots, &d_first));
    if (match_count) GK_TRY_HIP(c, scratch(c, "match_count", cap_slots, &d_count));
    // the pinned staging's two slots (stage_reserve), as gk_screen's: bytes in, the per-position arrays
    // that were asked for out, each chunk's results leaving their slot two chunks later
    auto pad = [](uint64_t b) { return (b + 255) / 256 * 256; };
    const uint64_t b_bytes = pad(cap_bytes);
    const uint64_t l_bytes = match_len ? pad(4 * cap_slots) : 0, f_bytes = match_first ? pad(8 * cap_slots) : 0,
                   c_bytes = match_count ? pad(4 * cap_slots) : 0;
    const uint64_t o_len = b_bytes, o_first = o_len + l_bytes, o_count = o_first + f_bytes, o_bad = o_count + c_bytes;
    const uint64_t slot_bytes = o_bad + 256;  // (the last 256: the chunk's copy of d_bad)
    if (int rc = stage_reserve(c, slot_bytes)) return rc;

    GK_TRY_HIP(c, hipMemcpyAsync(d_off, offsets, 8 * (nseq + 1), hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_sum, 0, 8 * nseq, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_best, 0, 8 * nseq, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_bad, 0xFF, 8, c->stream));

    MatchArgs a{};
    a.bytes = d_bytes;
    a.offsets = d_off;
    a.nseq = nseq;
    a.K = c->sort_len;
    a.C = C;
    a.keys = c->keys[c->cur];
    a.dir = dir;
    a.D = c->lookup_dir_bits;
    a.sba = c->sba;
    a.starts = c->vals[c->cur];
    a.n = c->n;
    a.sum = d_sum;
    a.best = d_best;
    a.mlen = d_len;
    a.mfirst = d_first;
    a.mcount = d_count;
    a.bad = d_bad;
    const uint64_t nchunks = screen::chunk_count(total, chunk, C);
    auto drain = [&](uint64_t ci) {  // (after stage_ev[slot] or a stream sync)
        uint64_t start, nslots, nbytes;
        screen::chunk_range(total, chunk, C, ci, &start, &nslots, &nbytes);
        const uint8_t *slot = c->stage_pin + (ci & 1) * slot_bytes;
        if (match_len) std::memcpy(match_len + start, slot + o_len, 4 * nslots);
        if (match_first) std::memcpy(match_first + start, slot + o_first, 8 * nslots);
        if (match_count) std::memcpy(match_count + start, slot + o_count, 4 * nslots);
    };
    const char *timer_name = use_keys ? "match_keys" : "match_bytes";
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
        uint64_t start, nslots, nbytes;
        screen::chunk_range(total, chunk, C, ci, &start, &nslots, &nbytes);
        uint8_t *slot = c->stage_pin + (ci & 1) * slot_bytes;
        if (ci >= 2) {  // the slot's previous chunk: wait for it and hand its results over
            GK_TRY_HIP(c, hipEventSynchronize(c->stage_ev[ci & 1]));
            unsigned long long seen;  // a byte outside the alphabet so far: launch nothing more
            std::memcpy(&seen, slot + o_bad, 8);
            if (seen != ~0ull) break;
            drain(ci - 2);
        }
        std::memcpy(slot, seqs + start, nbytes);
        GK_TRY_HIP(c, hipMemcpyAsync(d_bytes, slot, nbytes, hipMemcpyHostToDevice, c->stream));
        a.base = start;
        a.nslots = nslots;
        a.nbytes = nbytes;
        const dim3 grid((unsigned)((nslots + kMatchTile - 1) / kMatchTile)), block(kMatchThreads);
        int tslot;
        timer_begin(c, timer_name, &tslot);
        timer_units(c, tslot, nslots);
        if (use_keys) hipLaunchKernelGGL(match_kernel<true>, grid, block, 0, c->stream, a);
        else hipLaunchKernelGGL(match_kernel<false>, grid, block, 0, c->stream, a);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, tslot);
        if (match_len)
            GK_TRY_HIP(c, hipMemcpyAsync(slot + o_len, d_len, 4 * nslots, hipMemcpyDeviceToHost, c->stream));
        if (match_first)
            GK_TRY_HIP(c, hipMemcpyAsync(slot + o_first, d_first, 8 * nslots, hipMemcpyDeviceToHost, c->stream));
        if (match_count)
            GK_TRY_HIP(c, hipMemcpyAsync(slot + o_count, d_count, 4 * nslots, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(slot + o_bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipEventRecord(c->stage_ev[ci & 1], c->stream));
    }
    // the smallest bad position of the chunks launched: the chunks run in order, so it is the batch's
    unsigned long long bad = 0;
    GK_TRY_HIP(c, read_back(c, d_bad, 8, &bad));  // (synchronises the stream)
    if (bad != ~0ull) {
        uint64_t seq, off;
        screen::locate(offsets, nseq, bad, &seq, &off);
        const uint8_t b = seqs[bad];
        char msg[200];
        std::snprintf(msg, sizeof msg,
                      "sequence %llu holds byte 0x%02x ('%c') at offset %llu, outside the alphabet ABCDGHKMNRSTVWY",
                      (unsigned long long)seq, (unsigned)b, (b >= 32 && b < 127) ? (char)b : '?',
                      (unsigned long long)off);
        return fail(c, GK_E_ALPHABET, msg);
    }
    if (nchunks >= 2) drain(nchunks - 2);
    drain(nchunks - 1);
    // the per-sequence accumulators, once: sum_len as it is, the packed maximum taken apart
    GK_TRY_HIP(c, hipMemcpy(sum_len, d_sum, 8 * nseq, hipMemcpyDeviceToHost));
    std::vector<uint64_t> best(nseq);
    GK_TRY_HIP(c, hipMemcpy(best.data(), d_best, 8 * nseq, hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < nseq; ++j) {
        longest[j] = match::best_len(best[j]);
        longest_pos[j] = match::best_pos(best[j]);
    }
    return GK_OK;
}
