// gkm_screen.hip -- gk_screen: how much of each read of a batch is in the sorted index (gfx950).
//
// For every window of K bytes (K = the sort length) inside one sequence of the batch, the window's
// count is what gk_lookup returns as `count` for those bytes; per sequence the device sums the counts
// and the windows with a count above 0 ("Screen").  Each base crosses the link once: the
// batch goes over in chunks that overlap by K - 1 bytes, the windows are formed on the device.
// Two paths, the same answers, as in gk_lookup:
//   keys   final one-word 2-bit keys in sorted order: a block stages a tile of positions plus a K - 1
//          halo in LDS as 2-bit codes and flags, a thread builds the key of its first window and rolls
//          the following ones, and its windows' searches (key_search, gkm_lookup_search.h: gk_lookup's)
//          advance in lockstep.  A window with a letter other than A, C, G, T counts 0 unsearched: the
//          index is A/C/G/T-only.
//   bytes  one search per window over the sorted starts, comparing sba bytes with the read's in 4-bit
//          codes; canonical orders compare canonical forms on both sides.  Always valid.  The search
//          and the comparison are gkm_bytes_search.h's (gk_lookup's and gk_join's), the window read
//          in place; a byte outside the alphabet in it is code 0 and fails the call.
// (gkm_tile_seqs.h, shared with gk_match:) A tile finds the sequences of its first and last position by a search over `offsets` that the 64
// lanes of one wave share, keeps the boundaries between them in LDS (kScreenBounds at a time: a tile
// with more -- many empty or very short reads -- takes them in several passes), sums per sequence in
// LDS and issues one global atomic per (block, sequence) and counter.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "gkm_bytes_search.h"
#include "gkm_internal.h"
#include "gkm_lookup_search.h"
#include "gkm_screen_host.h"
#include "gkm_tile_seqs.h"

#ifndef GKM_SCREEN_WIN
// windows per thread: 2, 4 and 8 measured within the run-to-run spread of one another at C3 size
// (profiles/screen/ab_windows_per_thread.txt)
#define GKM_SCREEN_WIN 4
#endif

namespace gkm {

constexpr int kScreenThreads = 256;
constexpr int kScreenWin = GKM_SCREEN_WIN;
constexpr int kScreenTile = kScreenThreads * kScreenWin;  // positions per block
// sequence ends a pass keeps in LDS.  The table against a per-thread search of `offsets` in device
// memory has not been measured against each other: the table is unmeasured
constexpr int kScreenBounds = 256;
constexpr int kScreenHalo = 31;                           // key path: K <= 32

struct ScreenArgs {
    const uint8_t *bytes;     // the chunk: bytes [base, base + nbytes) of the batch
    uint64_t base, nslots, nbytes;  // the chunk owns the positions [base, base + nslots)
    const uint64_t *offsets;  // [nseq + 1]
    uint64_t nseq;
    uint32_t K;
    int both;                 // GK_SCREEN_BOTH_STRANDS on a forward order
    const uint64_t *keys;     // key path
    const uint32_t *dir;
    int D;
    const uint8_t *sba;       // byte path
    const uint32_t *starts;
    uint64_t n;
    uint32_t *present;              // [nseq]
    unsigned long long *occ;        // [nseq]
    uint32_t *wc;                   // [nslots] or null
    unsigned long long *bad;        // smallest position of a byte outside the alphabet
};

// sign of (reverse complement of q) - q over K symbols in 4-bit codes
__device__ __forceinline__ int rc_sign(const uint8_t *__restrict__ q, int K, const uint8_t *lut4) {
    for (int t = 0; t < K; ++t) {
        const uint32_t f = lut4[q[t]], r = comp_sym<4>(lut4[q[K - 1 - t]]);
        if (f != r) return r < f ? -1 : 1;
    }
    return 0;
}

// MODE 0: keys, 1: bytes, 2: bytes of a canonical order.  One block per tile of kScreenTile positions.
template <int MODE>
__global__ __launch_bounds__(kScreenThreads) void screen_kernel(const ScreenArgs a) {
    constexpr int W = kScreenWin;
    __shared__ uint8_t s_lut4[256];
    // key path: per position, bits 0-1 the 2-bit code, bit 2 "not A/C/G/T"
    __shared__ uint8_t s_code[MODE == 0 ? kScreenTile + kScreenHalo : 1];
    __shared__ uint64_t s_tab[kScreenBounds];  // ends of the pass's sequences
    __shared__ unsigned long long s_occ[kScreenBounds];
    __shared__ uint32_t s_pres[kScreenBounds];
    __shared__ uint64_t s_j[2];
    const int tid = threadIdx.x;
    const int K = (int)a.K;
    s_lut4[tid] = code4(tid);
    const uint64_t t0 = blockIdx.x * (uint64_t)kScreenTile;  // in the chunk
    const uint64_t t1 = t0 + kScreenTile < a.nslots ? t0 + kScreenTile : a.nslots;
    const uint64_t g0 = a.base + t0, g1 = a.base + t1;       // in the batch
    if (tid < 64) tile_seq_span(a.offsets, a.nseq, g0, g1, tid, s_j);  // the tile's first and last sequence
    __syncthreads();
    // the alphabet check of the positions the tile owns; the key path's staging with its halo
    if (MODE == 0) {
        const uint64_t have = a.nbytes - t0;
        for (int i = tid; i < kScreenTile + K - 1; i += kScreenThreads) {
            uint8_t v = 4;  // past the chunk: no window that counts reaches here
            if ((uint64_t)i < have) {
                const uint32_t b = a.bytes[t0 + i];
                const bool acgt = (b == 'A') | (b == 'C') | (b == 'G') | (b == 'T');
                v = acgt ? (uint8_t)canon_code<2>(b, nullptr) : (uint8_t)4;
                if ((uint64_t)i < t1 - t0 && s_lut4[b] == 0) atomicMin(a.bad, (unsigned long long)(g0 + i));
            }
            s_code[i] = v;
        }
    } else {
        for (int i = tid; (uint64_t)i < t1 - t0; i += kScreenThreads)
            if (s_lut4[a.bytes[t0 + i]] == 0) atomicMin(a.bad, (unsigned long long)(g0 + i));
    }
    const uint64_t j0 = s_j[0], j1 = s_j[1];
    const uint64_t pt0 = g0 + (uint64_t)tid * W;  // this thread's run of positions
    const uint64_t pt1 = pt0 + W < g1 ? pt0 + W : g1;
    const uint64_t mask = K >= 32 ? ~0ull : (1ull << (2 * K)) - 1;
    auto init = [&](int i) {
        s_pres[i] = 0;
        s_occ[i] = 0;
    };
    auto body = [&](uint64_t, int cnt, uint64_t slab_lo, uint64_t slab_hi) {
        const uint64_t pa = slab_lo > pt0 ? slab_lo : pt0, pb = slab_hi < pt1 ? slab_hi : pt1;
        if (pa < pb) {
            int jr = pass_seq_of(s_tab, cnt, pa);  // the sequence of pa in the pass
            const int m = (int)(pb - pa);
            int cur = jr;
            uint32_t pres = 0;
            unsigned long long occ = 0;
            auto flush = [&]() {
                if (pres) atomicAdd(&s_pres[cur], pres);
                if (occ) atomicAdd(&s_occ[cur], occ);
            };
            if (MODE == 0) {
                const int li = (int)(pa - g0);
                uint64_t key = 0, rck = 0;
                int clean = 0;  // A/C/G/T codes in a row up to the window's last
                for (int t = 0; t < K; ++t) {
                    const uint32_t c = s_code[li + t];
                    key = (key << 2) | (c & 3);
                    clean = (c & 4) ? 0 : clean + 1;
                }
                if (a.both) rck = revcomp_word<2>(key, K);
                uint64_t pk[W], rk[W], f[W];
                uint32_t c1[W], c2[W];
                bool act[W], act2[W];
                int sj[W];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    pk[w] = rk[w] = 0;
                    act[w] = act2[w] = false;
                    sj[w] = 0;
                    c2[w] = 0;
                    if (w >= m) continue;
                    if (w > 0) {
                        const uint32_t c = s_code[li + K - 1 + w];
                        key = ((key << 2) | (c & 3)) & mask;
                        rck = (rck >> 2) | ((uint64_t)(3 - (c & 3)) << (2 * (K - 1)));
                        clean = (c & 4) ? 0 : clean + 1;
                    }
                    const uint64_t p = pa + w;
                    while (s_tab[jr] <= p) ++jr;
                    sj[w] = jr;
                    const bool ok = clean >= K && p + K <= s_tab[jr];
                    pk[w] = key;
                    rk[w] = rck;
                    act[w] = ok;
                    act2[w] = ok && a.both && rck != key;  // its own reverse complement: once
                }
                key_search<W>(a.keys, a.n, a.dir, a.D, 2 * K, 0, pk, act, f, c1);
                if (a.both) key_search<W>(a.keys, a.n, a.dir, a.D, 2 * K, 0, rk, act2, f, c2);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w >= m) continue;
                    const uint32_t cw = c1[w] + c2[w];
                    if (a.wc) a.wc[pa + w - a.base] = cw;
                    if (sj[w] != cur) {
                        flush();
                        cur = sj[w];
                        pres = 0;
                        occ = 0;
                    }
                    pres += cw > 0;
                    occ += cw;
                }
            } else {
                for (uint64_t p = pa; p < pb; ++p) {
                    while (s_tab[jr] <= p) ++jr;
                    uint32_t cw = 0;
                    if (p + K <= s_tab[jr]) {
                        const uint8_t *q = a.bytes + (p - a.base);
                        const int s = (MODE == 2 || a.both) ? rc_sign(q, K, s_lut4) : 0;
                        // the window's count (gkm_bytes_search.h), the window read in place: its
                        // canonical form on a canonical order, its other strand too if a.both
                        uint64_t f;
                        bytes_range<MODE == 2>(a.sba, a.starts, a.n, K, s_lut4,
                                               SoughtStrand{q, s_lut4, K, MODE == 2 && s < 0}, &f, &cw);
                        if (MODE == 1 && a.both && s != 0) {
                            uint32_t cr;
                            bytes_range<false>(a.sba, a.starts, a.n, K, s_lut4, SoughtStrand{q, s_lut4, K, true}, &f, &cr);
                            cw += cr;
                        }
                    }
                    if (a.wc) a.wc[p - a.base] = cw;
                    if (jr != cur) {
                        flush();
                        cur = jr;
                        pres = 0;
                        occ = 0;
                    }
                    pres += cw > 0;
                    occ += cw;
                }
            }
            flush();
        }
    };
    auto flush_seq = [&](int i, uint64_t j) {
        if (s_pres[i]) atomicAdd(&a.present[j], s_pres[i]);
        if (s_occ[i]) atomicAdd(&a.occ[j], s_occ[i]);
    };
    tile_seq_passes<kScreenBounds, kScreenThreads>(a.offsets, j0, j1, g0, g1, s_tab, tid, init, body, flush_seq);
}

}  // namespace gkm

using namespace gkm;

extern "C" int gk_screen(gk_ctx *c, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t flags,
                         uint32_t *n_present, uint64_t *occurrences, uint32_t *window_count) {
    if (!c) return GK_E_ARG;
    if (nseq == 0) return GK_OK;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (!c->have_starts || !c->sorted) return fail(c, GK_E_STATE, "the k-mers are not sorted: call gk_sort first");
    if (c->sort_len == 0)
        return fail(c, GK_E_UNSUPPORTED, "gk_screen needs a sort with a fixed max_kmer_len (the windows' length)");
    if (!offsets || !n_present || !occurrences) return fail(c, GK_E_ARG, "null array");
    if (flags & ~GK_SCREEN_BOTH_STRANDS) return fail(c, GK_E_ARG, "unknown flag bits");
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
    const uint32_t K = c->sort_len;
    if (total == 0) {
        std::memset(n_present, 0, 4 * nseq);
        std::memset(occurrences, 0, 8 * nseq);
        return GK_OK;
    }
    if (!seqs) return fail(c, GK_E_ARG, "null array");
    // path: the keys when the context holds final 2-bit keys (an A/C/G/T-only index: a window with any
    // other letter counts 0 there), else the bytes
    const bool keys_ok = lookup_keys_usable(c);
    bool use_keys = keys_ok;
    const int path = query::parse_path(opt("GKM_SCREEN_PATH"));
    if (path < 0) return fail(c, GK_E_ARG, "GKM_SCREEN_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !keys_ok)
        return fail(c, GK_E_UNSUPPORTED, "GKM_SCREEN_PATH=keys: the context holds no final one-word 2-bit forward keys");
    if (path == query::kPathBytes) use_keys = false;
    const uint64_t chunk = screen::chunk_bytes(opt("GKM_SCREEN_CHUNK"), K);
    const uint64_t step = screen::chunk_step(chunk, K);

    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (int rc = materialize_starts(c)) return rc;
    uint32_t *dir = nullptr;
    if (use_keys)
        if (int rc = lookup_build_dir(c, &dir)) return rc;

    const uint64_t cap_bytes = std::min(chunk, total), cap_slots = std::min(step, total);
    uint8_t *d_bytes;
    uint64_t *d_off;
    uint32_t *d_present, *d_wc = nullptr;
    unsigned long long *d_occ, *d_bad;
    GK_TRY_HIP(c, scratch(c, "screen_bytes", cap_bytes, &d_bytes));
    GK_TRY_HIP(c, scratch(c, "screen_off", nseq + 1, &d_off));
    GK_TRY_HIP(c, scratch(c, "screen_present", nseq, &d_present));
    GK_TRY_HIP(c, scratch(c, "screen_occ", nseq, &d_occ));
    GK_TRY_HIP(c, scratch(c, "screen_bad", 1, &d_bad));
    if (window_count) GK_TRY_HIP(c, scratch(c, "screen_wc", cap_slots, &d_wc));
    // the pinned staging's two slots (stage_reserve): the host fills slot s while the copy engine and
    // the kernel work on slot s ^ 1, and a chunk's window counts leave their slot for the caller's
    // array two chunks later
    const uint64_t b_bytes = (cap_bytes + 255) / 256 * 256;
    const uint64_t w_bytes = window_count ? (4 * cap_slots + 255) / 256 * 256 : 0;
    const uint64_t slot_bytes = b_bytes + w_bytes + 256;  // (the last 256: the chunk's copy of d_bad)
    if (int rc = stage_reserve(c, slot_bytes)) return rc;

    GK_TRY_HIP(c, hipMemcpyAsync(d_off, offsets, 8 * (nseq + 1), hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_present, 0, 4 * nseq, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_occ, 0, 8 * nseq, c->stream));
    GK_TRY_HIP(c, hipMemsetAsync(d_bad, 0xFF, 8, c->stream));

    ScreenArgs a{};
    a.bytes = d_bytes;
    a.offsets = d_off;
    a.nseq = nseq;
    a.K = K;
    a.both = (flags & GK_SCREEN_BOTH_STRANDS) && !c->canonical;
    a.keys = c->keys[c->cur];
    a.dir = dir;
    a.D = c->lookup_dir_bits;
    a.sba = c->sba;
    a.starts = c->vals[c->cur];
    a.n = c->n;
    a.present = d_present;
    a.occ = d_occ;
    a.wc = d_wc;
    a.bad = d_bad;
    const uint64_t nchunks = screen::chunk_count(total, chunk, K);
    auto drain = [&](uint64_t ci) {  // (after stage_ev[slot] or a stream sync)
        if (!window_count) return;
        uint64_t start, nslots, nbytes;
        screen::chunk_range(total, chunk, K, ci, &start, &nslots, &nbytes);
        std::memcpy(window_count + start, c->stage_pin + (ci & 1) * slot_bytes + b_bytes, 4 * nslots);
    };
    const char *timer_name = use_keys ? "screen_keys" : "screen_bytes";
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
        uint64_t start, nslots, nbytes;
        screen::chunk_range(total, chunk, K, ci, &start, &nslots, &nbytes);
        uint8_t *slot = c->stage_pin + (ci & 1) * slot_bytes;
        if (ci >= 2) {  // the slot's previous chunk: wait for it and hand its counts over
            GK_TRY_HIP(c, hipEventSynchronize(c->stage_ev[ci & 1]));
            unsigned long long seen;  // a byte outside the alphabet so far: launch nothing more
            std::memcpy(&seen, slot + b_bytes + w_bytes, 8);
            if (seen != ~0ull) break;
            drain(ci - 2);
        }
        std::memcpy(slot, seqs + start, nbytes);
        GK_TRY_HIP(c, hipMemcpyAsync(d_bytes, slot, nbytes, hipMemcpyHostToDevice, c->stream));
        a.base = start;
        a.nslots = nslots;
        a.nbytes = nbytes;
        const dim3 grid((unsigned)((nslots + kScreenTile - 1) / kScreenTile)), block(kScreenThreads);
        int tslot;
        timer_begin(c, timer_name, &tslot);
        timer_units(c, tslot, nslots);
        if (use_keys) hipLaunchKernelGGL(screen_kernel<0>, grid, block, 0, c->stream, a);
        else if (c->canonical) hipLaunchKernelGGL(screen_kernel<2>, grid, block, 0, c->stream, a);
        else hipLaunchKernelGGL(screen_kernel<1>, grid, block, 0, c->stream, a);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, tslot);
        if (window_count)
            GK_TRY_HIP(c, hipMemcpyAsync(slot + b_bytes, d_wc, 4 * nslots, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(slot + b_bytes + w_bytes, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
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
    GK_TRY_HIP(c, hipMemcpy(n_present, d_present, 4 * nseq, hipMemcpyDeviceToHost));
    GK_TRY_HIP(c, hipMemcpy(occurrences, d_occ, 8 * nseq, hipMemcpyDeviceToHost));
    return GK_OK;
}
