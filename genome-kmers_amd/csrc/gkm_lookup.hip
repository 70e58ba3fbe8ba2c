// gkm_lookup.hip -- gk_lookup: batch k-mer lookup in the sorted index (gfx950).
//
// A query of q bytes matches sorted position i when compare_sba_kmers_lexicographically(sba, query,
// starts[i], 0, max_kmer_len=q) is 0 (kmers.py:306-397); the sorted order is monotone under that
// comparison for every q <= the sort length, so the matches are one range [first, first + count).
// Two paths, the same answers ("Lookup"):
//   bytes  one thread per query: lower and upper bound over the sorted starts, comparing the sba bytes
//          at starts[mid] with the query in 4-bit symbol codes ('$' / end = 0, below every letter);
//          canonical orders compare the k-mer's canonical form.  Always valid.  The search and the
//          comparison are gkm_bytes_search.h's, shared with gk_join and gk_screen.
//   keys   final one-word 2-bit keys in sorted order and A/C/G/T-only queries: the query becomes its
//          2 q-bit prefix and the search runs over keys[cur] >> shift, inside the bucket a prefix
//          directory of the top D key bits gives (built by the first such lookup after a sort).
// Both are dependent gathers, bound by memory latency: 256-thread blocks, grid-stride, one query per
// thread and step, as b_group_pos_kernel (gkm_split.hip).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "gkm_bytes_search.h"
#include "gkm_internal.h"
#include "gkm_lookup_host.h"
#include "gkm_lookup_search.h"

namespace gkm {

constexpr int kLookupThreads = 256;
constexpr int kLookupMaxBlocks = 2048;      // 8 blocks per CU; the rest by grid stride
constexpr uint32_t kLookupLdsQlen = 192;    // longer queries stay in device memory (48 KiB of LDS per block)
constexpr int kLookupDirBits = 22;          // 4 Mi buckets, 16 MiB of uint32

// ---------------------------------------------------------------------------------------------
// byte path
// ---------------------------------------------------------------------------------------------
// bytes_range (gkm_bytes_search.h); the query's codes: this thread's column of the block's LDS copy
// when LDS (SoughtLds strides it by 256), else lut4 of the query bytes where they lie
static_assert(kLookupThreads == 256);
template <bool CANON, bool LDS>
__global__ __launch_bounds__(kLookupThreads) void lookup_bytes_kernel(
    const uint8_t *__restrict__ sba, const uint32_t *__restrict__ starts, uint64_t n,
    const uint8_t *__restrict__ queries, uint64_t m, uint32_t qlen, uint64_t *__restrict__ first,
    uint32_t *__restrict__ count) {
    extern __shared__ uint8_t s_query[];  // LDS: [qlen][256] symbol codes, one column per thread
    __shared__ uint8_t s_lut4[256];
    s_lut4[threadIdx.x] = code4(threadIdx.x);
    __syncthreads();
    for (uint64_t i = blockIdx.x * (uint64_t)kLookupThreads + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * kLookupThreads) {
        const uint8_t *qg = queries + i * qlen;
        const int q = (int)qlen;
        if (LDS)  // (a thread reads back only the column it wrote: no barrier)
            for (uint32_t t = 0; t < qlen; ++t) s_query[t * kLookupThreads + threadIdx.x] = s_lut4[qg[t]];
        if (LDS) bytes_range<CANON>(sba, starts, n, q, s_lut4, SoughtLds{s_query + threadIdx.x}, &first[i], &count[i]);
        else bytes_range<CANON>(sba, starts, n, q, s_lut4, SoughtBytes{qg, s_lut4}, &first[i], &count[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// key path
// ---------------------------------------------------------------------------------------------
// dir[d] = number of keys whose top D bits (key >> sd) are below d, for d in [0, 1 << D]; the last
// entry is n (n <= 2^32 - 1 fits the uint32)
__global__ __launch_bounds__(kLookupThreads) void lookup_dir_kernel(const uint64_t *__restrict__ keys, uint64_t n,
                                                                    int D, int sd, uint32_t *__restrict__ dir) {
    const uint64_t entries = (1ull << D) + 1;
    for (uint64_t d = blockIdx.x * (uint64_t)kLookupThreads + threadIdx.x; d < entries;
         d += (uint64_t)gridDim.x * kLookupThreads) {
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((keys[mid] >> sd) < d) lo = mid + 1;
            else hi = mid;
        }
        dir[d] = (uint32_t)lo;
    }
}

// keys: n one-word keys of `symbols` 2-bit symbols, ascending; dir (may be null): the directory of the
// top D bits above.  The search itself is key_search (gkm_lookup_search.h), shared with gk_screen.
__global__ __launch_bounds__(kLookupThreads) void lookup_keys_kernel(
    const uint64_t *__restrict__ keys, uint64_t n, int symbols, const uint32_t *__restrict__ dir, int D,
    const uint8_t *__restrict__ queries, uint64_t m, uint32_t qlen, uint64_t *__restrict__ first,
    uint32_t *__restrict__ count) {
    const int qb = 2 * (int)qlen;
    const int shift = 2 * (symbols - (int)qlen);
    for (uint64_t i = blockIdx.x * (uint64_t)kLookupThreads + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * kLookupThreads) {
        const uint8_t *qg = queries + i * qlen;
        uint64_t prefix[1] = {0};
        for (uint32_t t = 0; t < qlen; ++t) prefix[0] = (prefix[0] << 2) | canon_code<2>(qg[t], nullptr);
        const bool active[1] = {true};
        uint64_t f[1];
        uint32_t cnt[1];
        key_search<1>(keys, n, dir, D, qb, shift, prefix, active, f, cnt);
        first[i] = f[0];
        count[i] = cnt[0];
    }
}

static unsigned lookup_grid(uint64_t items) {
    const uint64_t g = (items + kLookupThreads - 1) / kLookupThreads;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), kLookupMaxBlocks);
}

int lookup_build_dir(gk_ctx *c, uint32_t **out) {
    const int D = std::min(kLookupDirBits, 2 * c->spec.symbols);
    const uint64_t entries = (1ull << D) + 1;
    uint32_t *dir;
    GK_TRY_HIP(c, scratch(c, "lookup_dir", entries, &dir));
    if (!c->lookup_dir_valid || c->lookup_dir_bits != D) {
        int slot;
        timer_begin(c, "lookup_dir_build", &slot);
        timer_units(c, slot, entries);
        hipLaunchKernelGGL(lookup_dir_kernel, dim3(lookup_grid(entries)), dim3(kLookupThreads), 0, c->stream,
                           c->keys[c->cur], c->n, D, 2 * c->spec.symbols - D, dir);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        c->lookup_dir_valid = true;
        c->lookup_dir_bits = D;
    }
    *out = dir;
    return GK_OK;
}

// Pinned staging (grow-only, kept for the context's life): a copy from or to pageable memory is
// staged by the runtime at a fraction of the link's rate and holds the host meanwhile; with two
// pinned slots the host fills slot s while the copy engine and the kernel work on slot s ^ 1.
int stage_reserve(gk_ctx *c, uint64_t slot_bytes) {
    if (c->stage_pin_cap < 2 * slot_bytes) {
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        if (c->stage_pin) (void)hipHostFree(c->stage_pin);
        c->stage_pin = nullptr;
        c->stage_pin_cap = 0;
        GK_TRY_HIP(c, hipHostMalloc(reinterpret_cast<void **>(&c->stage_pin), 2 * slot_bytes, hipHostMallocDefault));
        c->stage_pin_cap = 2 * slot_bytes;
    }
    for (hipEvent_t &ev : c->stage_ev)
        if (!ev) GK_TRY_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return GK_OK;
}

int fail_alphabet(gk_ctx *c, const uint8_t *queries, uint64_t bad, uint32_t qlen) {
    const uint8_t b = queries[bad];
    char msg[160];
    std::snprintf(msg, sizeof msg, "query %llu holds byte 0x%02x ('%c') outside the alphabet ABCDGHKMNRSTVWY",
                  (unsigned long long)(bad / qlen), (unsigned)b, (b >= 32 && b < 127) ? (char)b : '?');
    return fail(c, GK_E_ALPHABET, msg);
}

}  // namespace gkm

using namespace gkm;

extern "C" int gk_lookup(gk_ctx *c, const uint8_t *queries, uint64_t m, uint32_t qlen, uint64_t *first,
                         uint32_t *count) {
    if (!c) return GK_E_ARG;
    if (m == 0) return GK_OK;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (!c->have_starts || !c->sorted) return fail(c, GK_E_STATE, "the k-mers are not sorted: call gk_sort first");
    if (!queries || !first || !count) return fail(c, GK_E_ARG, "null array");
    if (qlen == 0) return fail(c, GK_E_ARG, "query length must be greater than zero");
    if (c->sort_len != 0 && qlen > c->sort_len)
        return fail(c, GK_E_ARG, "query length (" + std::to_string(qlen) + ") is greater than the sort length (" +
                                     std::to_string(c->sort_len) + ")");
    if (c->canonical && qlen != c->sort_len)
        return fail(c, GK_E_ARG, "canonical k-mers are looked up at the sort length (" + std::to_string(c->sort_len) +
                                     ") only (query length = " + std::to_string(qlen) + ")");
    if (m > UINT64_MAX / qlen) return fail(c, GK_E_ARG, "query batch too large");
    bool all_acgt = false;
    const int64_t bad = lookup::validate_queries(queries, m, qlen, &all_acgt);
    if (bad >= 0) return fail_alphabet(c, queries, (uint64_t)bad, qlen);
    // path: the keys when the context holds final 2-bit keys and the queries are ACGT, else the bytes
    const bool keys_ok = lookup_keys_usable(c);
    bool use_keys = keys_ok && all_acgt;
    const int path = query::parse_path(opt("GKM_LOOKUP_PATH"));
    if (path < 0) return fail(c, GK_E_ARG, "GKM_LOOKUP_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !use_keys)
        return fail(c, GK_E_UNSUPPORTED,
                    keys_ok ? "GKM_LOOKUP_PATH=keys: a query holds a letter other than A, C, G, T"
                            : "GKM_LOOKUP_PATH=keys: the context holds no final one-word 2-bit forward keys");
    if (path == query::kPathBytes) use_keys = false;
    const char *dir_opt = opt("GKM_LOOKUP_DIR");
    const bool use_dir = !(dir_opt && std::strcmp(dir_opt, "0") == 0);
    const uint64_t chunk = lookup::chunk_size(opt("GKM_LOOKUP_CHUNK"), qlen);

    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (int rc = materialize_starts(c)) return rc;
    uint32_t *dir = nullptr;
    if (use_keys && use_dir)
        if (int rc = lookup_build_dir(c, &dir)) return rc;

    const uint64_t cap = std::min(chunk, m);
    uint8_t *d_q;
    uint64_t *d_first;
    uint32_t *d_count;
    GK_TRY_HIP(c, scratch(c, "lookup_q", cap * qlen, &d_q));
    GK_TRY_HIP(c, scratch(c, "lookup_first", cap, &d_first));
    GK_TRY_HIP(c, scratch(c, "lookup_count", cap, &d_count));
    // The pinned staging's two slots (stage_reserve; chunk_size bounds a slot at kChunk queries and
    // kChunkBytes of query bytes, so the block is at most ~150 MiB): the host fills slot s (a memcpy, or
    // the canonical form of each query) while the copy engine and the kernel work on slot s ^ 1, and a
    // chunk's results leave their slot for the caller's arrays two chunks later.
    const uint64_t q_bytes = (cap * qlen + 255) / 256 * 256, f_bytes = (8 * cap + 255) / 256 * 256;
    const uint64_t slot_bytes = q_bytes + f_bytes + (4 * cap + 255) / 256 * 256;
    if (int rc = stage_reserve(c, slot_bytes)) return rc;
    // a chunk's results, from its slot to the caller's arrays (after stage_ev[slot] or a stream sync)
    auto drain = [&](uint64_t ci) {
        uint64_t off, len;
        lookup::chunk_range(m, chunk, ci, &off, &len);
        const uint8_t *slot = c->stage_pin + (ci & 1) * slot_bytes;
        std::memcpy(first + off, slot + q_bytes, 8 * len);
        std::memcpy(count + off, slot + q_bytes + f_bytes, 4 * len);
    };
    const bool lds = qlen <= kLookupLdsQlen;
    const size_t shmem = lds ? (size_t)qlen * kLookupThreads : 0;
    const char *timer_name = !use_keys ? "lookup_bytes" : dir ? "lookup_keys_dir" : "lookup_keys";
    const uint64_t nchunks = lookup::chunk_count(m, chunk);
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
        uint64_t off, len;
        lookup::chunk_range(m, chunk, ci, &off, &len);
        uint8_t *slot = c->stage_pin + (ci & 1) * slot_bytes;
        if (ci >= 2) {  // the slot's previous chunk: wait for its results and hand them over
            GK_TRY_HIP(c, hipEventSynchronize(c->stage_ev[ci & 1]));
            drain(ci - 2);
        }
        const uint8_t *src = queries + off * qlen;
        if (c->canonical)  // min(query, reverse complement)
            for (uint64_t i = 0; i < len; ++i) lookup::canonical_query(src + i * qlen, qlen, slot + i * qlen);
        else
            std::memcpy(slot, src, len * qlen);
        GK_TRY_HIP(c, hipMemcpyAsync(d_q, slot, len * qlen, hipMemcpyHostToDevice, c->stream));
        const dim3 grid(lookup_grid(len)), block(kLookupThreads);
        int tslot;
        timer_begin(c, timer_name, &tslot);
        timer_units(c, tslot, len);
        if (use_keys) {
            hipLaunchKernelGGL(lookup_keys_kernel, grid, block, 0, c->stream, c->keys[c->cur], c->n, c->spec.symbols,
                               dir, c->lookup_dir_bits, d_q, len, qlen, d_first, d_count);
        } else {
            const uint8_t *sba = c->sba;
            const uint32_t *starts = c->vals[c->cur];
            if (c->canonical && lds)
                hipLaunchKernelGGL((lookup_bytes_kernel<true, true>), grid, block, shmem, c->stream, sba, starts, c->n,
                                   d_q, len, qlen, d_first, d_count);
            else if (c->canonical)
                hipLaunchKernelGGL((lookup_bytes_kernel<true, false>), grid, block, shmem, c->stream, sba, starts, c->n,
                                   d_q, len, qlen, d_first, d_count);
            else if (lds)
                hipLaunchKernelGGL((lookup_bytes_kernel<false, true>), grid, block, shmem, c->stream, sba, starts, c->n,
                                   d_q, len, qlen, d_first, d_count);
            else
                hipLaunchKernelGGL((lookup_bytes_kernel<false, false>), grid, block, shmem, c->stream, sba, starts,
                                   c->n, d_q, len, qlen, d_first, d_count);
        }
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, tslot);
        GK_TRY_HIP(c, hipMemcpyAsync(slot + q_bytes, d_first, 8 * len, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(slot + q_bytes + f_bytes, d_count, 4 * len, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipEventRecord(c->stage_ev[ci & 1], c->stream));
    }
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (nchunks >= 2) drain(nchunks - 2);
    drain(nchunks - 1);
    return GK_OK;
}
