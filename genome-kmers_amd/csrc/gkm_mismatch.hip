// gkm_mismatch.hip -- gk_lookup_mismatch: k-mer search with mismatches, a scan of every k-mer of the
// current order against a batch of queries (gfx950).
//
// Position i of the current start-index order is at distance d from a query of q bytes when the q
// bytes at starts[i] hold no '$' / end of the sba and differ from the query's in d places (plain byte
// inequality).  With GK_MISMATCH_BOTH_STRANDS the reverse complement of the query is a second
// comparison, reported as strand 1.  Two paths, the same answers ("Search with
// mismatches"):
//   keys   final one-word 2-bit keys (lookup_keys_usable), A/C/G/T-only queries, q <= the key's
//          symbols: k = key >> 2 (symbols - q), x = k ^ w, d = popcount((x | x >> 1) & 0x5555...)
//   bytes  everything else: the <= 32 bytes at sba + starts[i] once per launch into two words of
//          4-bit codes (a code 0, '$', among the first q marks the k-mer short: it takes no part),
//          x = k ^ w folded to one bit per nibble, d = popcount over both words
// One launch per chunk of queries is one pass over the k-mers: kMismatchR k-mers per thread in
// registers, the comparison index wave-uniform so that the encoded queries are scalar loads.  A hit is
// the rare outcome at the d this is built for: the hit test is one wave-uniform branch per comparison
// and kMismatchR k-mers; behind it the counts are 64-bit global atomics and the hit records one
// aggregated append per wave (ballot, lane prefix, one atomicAdd).  The host sorts the records.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gkm_internal.h"
#include "gkm_mismatch_host.h"

namespace gkm {

using mismatch::HitRecord;

constexpr int kMismatchThreads = 256;
constexpr int kMismatchR = 4;  // k-mers per thread
constexpr int kMismatchTile = kMismatchThreads * kMismatchR;
constexpr int kMismatchMaxBlocks = 2048;  // 8 blocks per CU; the rest by grid stride
constexpr uint64_t kMismatchRecFirst = 1ull << 20;  // hit records the first pass of a hits call has room for

// symbols that differ between two words of symbol codes, given x = their XOR: BITS = 2, the pairs of
// x that are not 00; BITS = 4, the nibbles that are not 0000.  On 32-bit halves (no symbol straddles
// them), so that the shifts are 32-bit ones.
template <int BITS>
__device__ __forceinline__ uint32_t differing_symbols(uint64_t x) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    lo |= lo >> 1;
    hi |= hi >> 1;
    if constexpr (BITS == 4) {
        lo |= lo >> 2;
        hi |= hi >> 2;
    }
    constexpr uint32_t kLow = BITS == 2 ? 0x55555555u : 0x11111111u;
    return (uint32_t)(__popc(lo & kLow) + __popc(hi & kLow));
}

// some nibble of v is 0000
__device__ __forceinline__ bool has_zero_nibble(uint64_t v) {
    return ((v - 0x1111111111111111ull) & ~v & 0x8888888888888888ull) != 0;
}

// distance of a k-mer (W words) to a query: W = 1, 2-bit codes; W = 2, 4-bit codes
template <int W>
__device__ __forceinline__ uint32_t mismatch_dist(const uint64_t *k, const uint64_t *w) {
    if constexpr (W == 1) return differing_symbols<2>(k[0] ^ w[0]);
    else return differing_symbols<4>(k[0] ^ w[0]) + differing_symbols<4>(k[1] ^ w[1]);
}

// W = 1: src_keys[i] >> shift is k-mer i's q-symbol prefix.  W = 2: the qlen bytes at sba + starts[i]
// (sba_len bytes, then the '$' pad).
// qw: E comparisons of W words each; comparison e is query (e >> sbit) of the chunk on strand
// e & ((1 << sbit) - 1).  counts: [queries of the chunk][maxd + 1], zeroed.  recs (may be null):
// room for rec_cap records, *rec_n the number appended so far (records past rec_cap are dropped,
// counted all the same).
template <int W>
__global__ __launch_bounds__(kMismatchThreads) void mismatch_kernel(
    const uint64_t *__restrict__ src_keys, int shift, const uint8_t *__restrict__ sba, uint64_t sba_len,
    const uint32_t *__restrict__ starts, uint64_t n, uint32_t qlen, const uint64_t *__restrict__ qw, uint32_t E,
    int sbit, uint32_t q_off, int maxd, unsigned long long *__restrict__ counts, HitRecord *__restrict__ recs,
    uint64_t rec_cap, unsigned long long *__restrict__ rec_n) {
    __shared__ uint8_t s_lut4[256];
    if (W == 2) {
        s_lut4[threadIdx.x] = code4(threadIdx.x);
        __syncthreads();
    }
    // W = 2: the nibbles of the first qlen symbols in each word (no shift by 64 at 16 symbols)
    const uint32_t n0 = qlen < 16 ? qlen : 16, n1 = qlen - n0;
    const uint64_t m0 = n0 == 16 ? ~0ull : (1ull << (4 * n0)) - 1, m1 = n1 == 16 ? ~0ull : (1ull << (4 * n1)) - 1;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tiles = (n + kMismatchTile - 1) / kMismatchTile;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t base = tile * kMismatchTile + threadIdx.x;
        uint64_t k[kMismatchR][W];
        int thr[kMismatchR];  // maxd, or -1 for a k-mer that takes no part (past n, or short)
#pragma unroll
        for (int r = 0; r < kMismatchR; ++r) {
            const uint64_t i = base + (uint64_t)r * kMismatchThreads;
            bool ok = i < n;
            // (a lane past n loads element n - 1, n >= 1, and drops it: the R loads of a tile are
            // unconditional, so they are in flight together)
            const uint64_t at = ok ? i : n - 1;
            if constexpr (W == 1) {
                k[r][0] = src_keys[at] >> shift;
            } else {
                // (whole 8-byte groups whatever qlen is: the sba's '$' pad keeps the reads in bounds)
                uint32_t start = starts[at];
                if (start >= sba_len) {  // (a caller's start past the end: no byte of it is read)
                    ok = false;
                    start = 0;
                }
                const uint8_t *p = sba + start;
                uint64_t w0 = 0, w1 = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if ((uint32_t)(8 * g) >= qlen) break;
                    uint64_t raw;
                    __builtin_memcpy(&raw, p + 8 * g, 8);
                    uint64_t codes = 0;
#pragma unroll
                    for (int b = 0; b < 8; ++b) codes |= (uint64_t)s_lut4[(raw >> (8 * b)) & 255u] << (4 * b);
                    if (g < 2) w0 |= codes << (32 * (g & 1));
                    else w1 |= codes << (32 * (g & 1));
                }
                // a code 0 among the first qlen symbols: the nibbles from qlen on are set before the test
                ok = ok && !has_zero_nibble(w0 | ~m0) && !has_zero_nibble(w1 | ~m1);
                k[r][0] = w0 & m0;
                k[r][1] = w1 & m1;
            }
            thr[r] = ok ? maxd : -1;
        }
        // (the next comparison's words are loaded one step ahead; the last step reads W words past
        // the E comparisons, inside the spare elements every scratch buffer ends with, and drops them)
        uint64_t w_next[W];
#pragma unroll
        for (int j = 0; j < W; ++j) w_next[j] = qw[j];
        for (uint32_t e = 0; e < E; ++e) {
            uint64_t w[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                w[j] = w_next[j];
                w_next[j] = qw[(uint64_t)(e + 1) * W + j];
            }
            int d[kMismatchR];
            bool any = false;
#pragma unroll
            for (int r = 0; r < kMismatchR; ++r) {
                d[r] = (int)mismatch_dist<W>(k[r], w);
                any = any || d[r] <= thr[r];
            }
            if (__ballot(any) == 0) continue;  // wave-uniform
            const uint32_t q_local = e >> sbit, strand = e & ((1u << sbit) - 1u);
#pragma unroll
            for (int r = 0; r < kMismatchR; ++r) {
                const bool hit = d[r] <= thr[r];
                const unsigned long long mask = __ballot(hit);
                if (mask == 0) continue;
                if (recs != nullptr) {
                    unsigned long long at = 0;
                    if (lane == 0) at = atomicAdd(rec_n, (unsigned long long)__popcll(mask));
                    at = __shfl(at, 0);
                    at += (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                    if (hit && at < rec_cap) {
                        HitRecord h;
                        h.kmer_num = base + (uint64_t)r * kMismatchThreads;
                        h.query = q_off + q_local;
                        h.mismatches = (uint16_t)d[r];
                        h.strand = (uint16_t)strand;
                        recs[at] = h;
                    }
                }
                if (hit) atomicAdd(&counts[(uint64_t)q_local * (uint32_t)(maxd + 1) + (uint32_t)d[r]], 1ull);
            }
        }
    }
}

}  // namespace gkm

using namespace gkm;

extern "C" int gk_lookup_mismatch(gk_ctx *c, const uint8_t *queries, uint64_t m, uint32_t qlen,
                                  uint32_t max_mismatches, uint32_t flags, uint64_t *counts, uint32_t *hit_query,
                                  uint64_t *hit_kmer_num, uint8_t *hit_mismatches, uint8_t *hit_strand,
                                  uint64_t capacity, uint64_t *n_hits) {
    if (!c) return GK_E_ARG;
    if (!n_hits) return fail(c, GK_E_ARG, "null n_hits");
    *n_hits = 0;
    if (m == 0) return GK_OK;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (!c->have_starts) return fail(c, GK_E_STATE, "no k-mers");
    if (!queries || !counts) return fail(c, GK_E_ARG, "null array");
    const bool want_hits = hit_query != nullptr;
    if (want_hits && (!hit_kmer_num || !hit_mismatches || !hit_strand)) return fail(c, GK_E_ARG, "null hit array");
    if (qlen == 0 || qlen > mismatch::kMaxQlen)
        return fail(c, GK_E_ARG, "query length (" + std::to_string(qlen) + ") must be between 1 and 32");
    if (max_mismatches > qlen)
        return fail(c, GK_E_ARG, "max_mismatches (" + std::to_string(max_mismatches) +
                                     ") is greater than the query length (" + std::to_string(qlen) + ")");
    if (flags & ~GK_MISMATCH_BOTH_STRANDS) return fail(c, GK_E_ARG, "unknown flag bits");
    if (m > (1ull << 32)) return fail(c, GK_E_ARG, "query batch too large");
    bool all_acgt = false;
    const int64_t bad = lookup::validate_queries(queries, m, qlen, &all_acgt);
    if (bad >= 0) return fail_alphabet(c, queries, (uint64_t)bad, qlen);
    // path: the keys when the context holds final 2-bit keys that cover qlen and the queries (and so
    // their complements) are ACGT, else the bytes
    const bool keys_ok = lookup_keys_usable(c) && qlen <= (uint32_t)c->spec.symbols;
    bool use_keys = keys_ok && all_acgt;
    const int path = query::parse_path(opt("GKM_MISMATCH_PATH"));
    if (path < 0) return fail(c, GK_E_ARG, "GKM_MISMATCH_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !use_keys)
        return fail(c, GK_E_UNSUPPORTED,
                    keys_ok ? "GKM_MISMATCH_PATH=keys: a query holds a letter other than A, C, G, T"
                            : "GKM_MISMATCH_PATH=keys: the context holds no final one-word 2-bit forward "
                              "keys of at least the query length");
    if (path == query::kPathBytes) use_keys = false;
    const uint32_t nd = max_mismatches + 1;
    if (c->n == 0) {
        std::memset(counts, 0, 8 * m * nd);
        return GK_OK;
    }
    const uint64_t chunk = mismatch::chunk_size(opt("GKM_MISMATCH_CHUNK"));
    const int sbit = (flags & GK_MISMATCH_BOTH_STRANDS) ? 1 : 0;
    const int W = use_keys ? 1 : 2;

    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (!use_keys)
        if (int rc = materialize_starts(c)) return rc;

    // every comparison's words, the whole batch (at most 32 bytes per query): chunk ci's are
    // [off << sbit, (off + len) << sbit) of them; the vector outlives the copies enqueued from it
    std::vector<uint64_t> qw((m << sbit) * W);
    for (uint64_t j = 0; j < m; ++j) {
        const uint8_t *q = queries + j * qlen;
        uint8_t rc[mismatch::kMaxQlen];
        for (int s = 0; s <= sbit; ++s) {
            if (s) mismatch::reverse_complement(q, qlen, rc);
            uint64_t *dst = qw.data() + ((j << sbit) + s) * W;
            if (use_keys) dst[0] = mismatch::encode2(s ? rc : q, qlen);
            else mismatch::encode4(s ? rc : q, qlen, dst);
        }
    }

    const uint64_t cap = std::min(chunk, m);
    uint64_t *d_qw;
    unsigned long long *d_counts, *d_nrec;
    GK_TRY_HIP(c, scratch(c, "mismatch_qw", (cap << sbit) * W, &d_qw));
    GK_TRY_HIP(c, scratch(c, "mismatch_counts", cap * nd, &d_counts));
    GK_TRY_HIP(c, scratch(c, "mismatch_nrec", 1, &d_nrec));

    const uint64_t tiles = (c->n + kMismatchTile - 1) / kMismatchTile;
    const dim3 grid((unsigned)std::min<uint64_t>(tiles, kMismatchMaxBlocks)), block(kMismatchThreads);
    const uint64_t nchunks = mismatch::chunk_count(m, chunk);
    // every chunk through the scan: the counts into the caller's array, the hit records (d_rec may be
    // null) into room for rec_cap of them
    auto scan = [&](HitRecord *d_rec, uint64_t rec_cap) -> int {
        GK_TRY_HIP(c, hipMemsetAsync(d_nrec, 0, 8, c->stream));
        for (uint64_t ci = 0; ci < nchunks; ++ci) {
            uint64_t off, len;
            mismatch::chunk_range(m, chunk, ci, &off, &len);
            const uint32_t E = (uint32_t)(len << sbit);
            GK_TRY_HIP(c, hipMemcpyAsync(d_qw, qw.data() + (off << sbit) * W, 8ull * E * W, hipMemcpyHostToDevice,
                                         c->stream));
            GK_TRY_HIP(c, hipMemsetAsync(d_counts, 0, 8 * len * nd, c->stream));
            int tslot;
            timer_begin(c, use_keys ? "mismatch_keys" : "mismatch_bytes", &tslot);
            timer_units(c, tslot, c->n * len);
            if (use_keys)
                hipLaunchKernelGGL(mismatch_kernel<1>, grid, block, 0, c->stream, c->keys[c->cur],
                                   2 * (c->spec.symbols - (int)qlen), nullptr, 0, nullptr, c->n, qlen, d_qw, E, sbit,
                                   (uint32_t)off, (int)max_mismatches, d_counts, d_rec, rec_cap, d_nrec);
            else
                hipLaunchKernelGGL(mismatch_kernel<2>, grid, block, 0, c->stream, nullptr, 0, c->sba, c->sba_len,
                                   c->vals[c->cur], c->n, qlen, d_qw, E, sbit, (uint32_t)off, (int)max_mismatches,
                                   d_counts, d_rec, rec_cap, d_nrec);
            GK_TRY_HIP(c, hipGetLastError());
            timer_end(c, tslot);
            GK_TRY_HIP(c, hipMemcpyAsync(counts + off * nd, d_counts, 8 * len * nd, hipMemcpyDeviceToHost,
                                         c->stream));
        }
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        return GK_OK;
    };
    // (a failed step leaves copies into the caller's counts enqueued: they are waited for before the
    // error goes back)
    auto scan_synced = [&](HitRecord *d_rec, uint64_t rec_cap) -> int {
        const int rc = scan(d_rec, rec_cap);
        if (rc != GK_OK) (void)hipStreamSynchronize(c->stream);
        return rc;
    };
    auto total_of = [&]() {
        uint64_t t = 0;
        for (uint64_t i = 0; i < m * nd; ++i) t += counts[i];
        return t;
    };
    // The record buffer is sized from what the scan finds, not from the caller's capacity: the first
    // pass has room for kMismatchRecFirst records (16 MiB, kept with the context's scratch); a search
    // with more hits scans once more into a buffer of exactly that many, released before returning.
    HitRecord *d_rec = nullptr;
    uint64_t rec_cap = 0;
    if (want_hits) {
        rec_cap = std::min(capacity, kMismatchRecFirst);
        GK_TRY_HIP(c, scratch(c, "mismatch_rec", rec_cap, &d_rec));
    }
    if (int rc = scan_synced(d_rec, rec_cap)) return rc;
    const uint64_t total = total_of();
    *n_hits = total;
    if (!want_hits) return GK_OK;
    if (capacity < total)
        return fail(c, GK_E_ARG, "capacity (" + std::to_string(capacity) + ") is smaller than the number of hits (" +
                                     std::to_string(total) + ")");
    const bool again = total > rec_cap;
    if (again) {
        if (total > UINT64_MAX / (2 * sizeof(HitRecord))) return fail(c, GK_E_OOM, "too many hits for one call");
        GK_TRY_HIP(c, scratch(c, "mismatch_rec_all", total, &d_rec));
        if (int rc = scan_synced(d_rec, total)) {
            scratch_release(c, "mismatch_rec_all");
            return rc;
        }
    }
    std::vector<HitRecord> rec(total);
    hipError_t copied = hipSuccess;
    if (total) {
        copied = hipMemcpyAsync(rec.data(), d_rec, sizeof(HitRecord) * total, hipMemcpyDeviceToHost, c->stream);
        if (copied == hipSuccess) copied = hipStreamSynchronize(c->stream);
    }
    if (again) scratch_release(c, "mismatch_rec_all");
    GK_TRY_HIP(c, copied);
    mismatch::sort_and_split(rec.data(), total, hit_query, hit_kmer_num, hit_mismatches, hit_strand);
    return GK_OK;
}
