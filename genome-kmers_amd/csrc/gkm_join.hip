// gkm_join.hip -- gk_join: the distinct k-mers of one sorted context looked up in another (gfx950).
//
// For entry u of A's unique view (gk_unique_counts: group start and multiplicity of each distinct
// k-mer of the sorted order) the join gives b_first[u] = the number of B's sorted k-mers that compare
// less and b_count[u] = the number that compare equal, under compare_sba_kmers_lexicographically at
// the common sort length K (kmers.py:306-397), of the canonical forms after GK_SORT_CANONICAL on both
// sides -- gk_lookup's convention with A's k-mers as the queries.  Two paths, the same answers
// ("Join"):
//   bytes  one thread per distinct k-mer of A: lower and upper bound over B's sorted starts, comparing
//          B's sba bytes with A's at its group head in 4-bit symbol codes, the canonical form of both
//          on canonical orders: gk_lookup's search (gkm_bytes_search.h).  Always valid.
//   keys   both contexts hold final one-word 2-bit forward keys of the same K (lookup_keys_usable): a
//          streaming merge join of the two unique views.  A partition kernel finds the merge-path
//          split of every tile boundary (gkm_join_host.h: diagonal_split, A first on a tie); a tile
//          kernel stages its slice of A's keys and of B's keys, group starts and multiplicities in
//          LDS -- B's slice plus the one element after it, where the match of the tile's last A
//          element can sit -- and answers each A element by a lower bound inside the staged B slice.
// Both reduce the four sums of gk_join_stats over the shared k-mers in integers (LDS atomics per
// block, one global atomic per block and sum): reproducible whatever the scheduling.
#include <algorithm>
#include "gkm_bytes_search.h"
#include "gkm_internal.h"
#include "gkm_join_host.h"
#include "gkm_query_host.h"

namespace gkm {

constexpr int kJoinThreads = 256;
constexpr int kJoinMaxBlocks = 2048;    // 8 blocks per CU; the rest by grid stride
constexpr uint32_t kJoinMaskTile = join::kTile;  // sorted positions per block and step of join_mask_kernel

// shared k-mers, their occurrences in A, in B, and the sum of the smaller of the two
struct JoinSums {
    uint64_t shared = 0, occ_a = 0, occ_b = 0, occ_min = 0;
    __device__ __forceinline__ void add(uint32_t ca, uint32_t cb) {
        shared += 1;
        occ_a += ca;
        occ_b += cb;
        occ_min += ca < cb ? ca : cb;
    }
};

// a block's sums into out[0, 4): s_sums is zero and visible to the block on entry
__device__ __forceinline__ void join_reduce(const JoinSums &t, unsigned long long *s_sums, unsigned long long *out) {
    if (t.shared) {
        atomicAdd(&s_sums[0], (unsigned long long)t.shared);
        atomicAdd(&s_sums[1], (unsigned long long)t.occ_a);
        atomicAdd(&s_sums[2], (unsigned long long)t.occ_b);
        atomicAdd(&s_sums[3], (unsigned long long)t.occ_min);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_sums[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_sums[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// byte path
// ---------------------------------------------------------------------------------------------
// bytes_range (gkm_bytes_search.h) over B's sorted starts, the sought k-mer A's at its group head in
// A's sba: its canonical form if CANON, its strand (rc_a) found once, outside the search.  Both
// k-mers are whole (gk_join refuses a side with k-mers cut short), so no symbol is a '$'.
template <bool CANON>
__global__ __launch_bounds__(kJoinThreads) void join_bytes_kernel(
    const uint8_t *__restrict__ sba_a, const uint32_t *__restrict__ starts_a, const uint32_t *__restrict__ heads_a,
    const uint32_t *__restrict__ count_a, uint64_t na, const uint8_t *__restrict__ sba_b,
    const uint32_t *__restrict__ starts_b, uint64_t n_b, int k, uint32_t *__restrict__ b_first,
    uint32_t *__restrict__ b_count, unsigned long long *__restrict__ sums) {
    __shared__ uint8_t s_lut4[256];
    __shared__ unsigned long long s_sums[4];
    s_lut4[threadIdx.x] = code4(threadIdx.x);
    if (threadIdx.x < 4) s_sums[threadIdx.x] = 0;
    __syncthreads();
    JoinSums t;
    for (uint64_t u = blockIdx.x * (uint64_t)kJoinThreads + threadIdx.x; u < na;
         u += (uint64_t)gridDim.x * kJoinThreads) {
        const uint8_t *pa = sba_a + starts_a[heads_a[u]];
        const bool rc_a = CANON && canon_is_rc<4>(pa, k, s_lut4);
        uint64_t lb;
        uint32_t cnt;
        bytes_range<CANON>(sba_b, starts_b, n_b, k, s_lut4, SoughtStrand{pa, s_lut4, k, rc_a}, &lb, &cnt);
        b_first[u] = (uint32_t)lb;  // (n_b <= 2^32 - 1: GK_E_LIMIT)
        b_count[u] = cnt;
        if (cnt) t.add(count_a[u], cnt);
    }
    join_reduce(t, s_sums, sums);
}

// ---------------------------------------------------------------------------------------------
// key path
// ---------------------------------------------------------------------------------------------
// splits[t] = the number of A elements among the first min(t * kTile, na + nb) merged elements, for
// t in [0, tiles]
__global__ __launch_bounds__(kJoinThreads) void join_partition_kernel(
    const uint64_t *__restrict__ ka, const uint32_t *__restrict__ ha, uint64_t na, const uint64_t *__restrict__ kb,
    const uint32_t *__restrict__ hb, uint64_t nb, uint64_t tiles, uint32_t *__restrict__ splits) {
    for (uint64_t t = blockIdx.x * (uint64_t)kJoinThreads + threadIdx.x; t <= tiles;
         t += (uint64_t)gridDim.x * kJoinThreads) {
        const uint64_t d = std::min(t * join::kTile, na + nb);
        splits[t] = (uint32_t)join::diagonal_split(ka, ha, na, kb, hb, nb, d);
    }
}

// Tile t holds A[i0, i1) and B[j0, j1), i0 + j0 = t * kTile, (i1 - i0) + (j1 - j0) <= kTile.  s_key:
// A's keys at [0, i1 - i0), then the keys of B[j0, j1 + ext) with ext = 1 while B goes on after the
// tile (kTile + 1 entries at most); s_head / s_cnt: group start and multiplicity of the same B
// elements.  The lower bound r of an A key among the staged B keys is inside the stage (the tie
// rule, gkm_join_host.h), except past B's end, where b_first is n_b; only staged entries are compared.
__global__ __launch_bounds__(kJoinThreads) void join_keys_kernel(
    const uint64_t *__restrict__ ka, const uint32_t *__restrict__ ha, const uint32_t *__restrict__ ca, uint64_t na,
    const uint64_t *__restrict__ kb, const uint32_t *__restrict__ hb, const uint32_t *__restrict__ cb, uint64_t nb,
    uint64_t n_b, uint64_t tiles, const uint32_t *__restrict__ splits, uint32_t *__restrict__ b_first,
    uint32_t *__restrict__ b_count, unsigned long long *__restrict__ sums) {
    __shared__ uint64_t s_key[join::kTile + 1];
    __shared__ uint32_t s_head[join::kTile + 1];
    __shared__ uint32_t s_cnt[join::kTile + 1];
    __shared__ unsigned long long s_sums[4];
    if (threadIdx.x < 4) s_sums[threadIdx.x] = 0;
    JoinSums acc;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t d0 = t * join::kTile, d1 = std::min(d0 + join::kTile, na + nb);
        const uint64_t i0 = splits[t], i1 = splits[t + 1];
        const uint64_t j0 = d0 - i0, j1 = d1 - i1;
        const uint32_t at = (uint32_t)(i1 - i0);
        const uint32_t bt = (uint32_t)(j1 - j0) + (j1 < nb ? 1u : 0u);
        __syncthreads();  // the previous tile's readers (and s_sums' zeroes)
        for (uint32_t x = threadIdx.x; x < at; x += kJoinThreads) s_key[x] = ka[ha[i0 + x]];
        for (uint32_t x = threadIdx.x; x < bt; x += kJoinThreads) {
            const uint32_t h = hb[j0 + x];
            s_key[at + x] = kb[h];
            s_head[x] = h;
            s_cnt[x] = cb[j0 + x];
        }
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < at; x += kJoinThreads) {
            const uint64_t key = s_key[x];
            const uint32_t r = join::lower_bound_u64(s_key + at, bt, key);
            uint32_t first = (uint32_t)n_b, cnt = 0;
            if (r < bt) {
                first = s_head[r];
                if (s_key[at + r] == key) cnt = s_cnt[r];
            }
            b_first[i0 + x] = first;
            b_count[i0 + x] = cnt;
            if (cnt) acc.add(ca[i0 + x], cnt);
        }
    }
    __syncthreads();
    join_reduce(acc, s_sums, sums);
}

// ---------------------------------------------------------------------------------------------
// mask
// ---------------------------------------------------------------------------------------------
// mask[i] = 1 when the k-mer at sorted position i has (b_count != 0) == keep_present.  One block per
// kJoinMaskTile positions and step: the groups that overlap them (at most kJoinMaskTile + 1, found by
// two searches over the group starts) are staged, and every position finds its group in the stage --
// the work per position is the same whether a group holds one position or a million.
__global__ __launch_bounds__(kJoinThreads) void join_mask_kernel(const uint32_t *__restrict__ heads,
                                                                 const uint32_t *__restrict__ b_count, uint64_t nu,
                                                                 uint64_t n, int keep_present,
                                                                 uint8_t *__restrict__ mask) {
    __shared__ uint32_t s_head[kJoinMaskTile + 1];
    __shared__ uint8_t s_flag[kJoinMaskTile + 1];
    const uint64_t tiles = (n + kJoinMaskTile - 1) / kJoinMaskTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t p0 = t * kJoinMaskTile, p1 = std::min(p0 + kJoinMaskTile, n);
        // groups [u0, u1): the one that holds p0 (heads[0] = 0, so u0 >= 0) up to the one that holds p1 - 1
        const uint64_t u0 = join::upper_bound_u32<uint64_t>(heads, nu, p0) - 1;
        const uint64_t u1 = join::upper_bound_u32<uint64_t>(heads, nu, p1 - 1);
        const uint32_t ng = (uint32_t)(u1 - u0);
        __syncthreads();  // the previous tile's readers
        for (uint32_t x = threadIdx.x; x < ng; x += kJoinThreads) {
            s_head[x] = heads[u0 + x];
            s_flag[x] = (uint8_t)((b_count[u0 + x] != 0) == (keep_present != 0));
        }
        __syncthreads();
        for (uint64_t p = p0 + threadIdx.x; p < p1; p += kJoinThreads)
            mask[p] = s_flag[join::upper_bound_u32<uint32_t>(s_head, ng, p) - 1];
    }
}

static unsigned join_grid(uint64_t items) {
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(items, 1), kJoinMaxBlocks);
}

// the unique view of c, computed if it is not valid; a context of fewer than two k-mers (which the
// sort leaves without keys, so gk_unique_counts refuses it) gets its trivial view here
static int join_unique(gk_ctx *c) {
    if (c->unique_valid) return GK_OK;
    if (c->n >= 2) return gk_unique_counts(c, nullptr);
    c->join_valid = false;
    if (c->n == 1) {
        if (int rc = materialize_starts(c)) return rc;
        GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->idx_b), &c->idx_b_cap, 4 * (c->n + 64)));
        GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->ucount), &c->ucount_cap, 4 * (c->n + 64)));
        const uint32_t one = 1;
        GK_TRY_HIP(c, hipMemsetAsync(c->idx_b, 0, 4, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(c->ucount, &one, 4, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->n_unique = c->n;
    c->unique_valid = true;
    return GK_OK;
}

static bool join_is_valid(const gk_ctx *c) { return c->join_valid && c->unique_valid; }

}  // namespace gkm

using namespace gkm;

extern "C" int gk_join(gk_ctx *a, gk_ctx *b, uint32_t flags, gk_join_stats *stats) {
    if (!a || !b) return a ? fail(a, GK_E_ARG, "gk_join: null context b") : GK_E_ARG;
    pre_drop(a);  // (the k-mer buffers: a prefetched L0 does not survive)
    pre_drop(b);
    a->join_valid = false;
    if (a->device != b->device)
        return fail(a, GK_E_ARG, "gk_join: the contexts are on different devices (a: " + std::to_string(a->device) +
                                     ", b: " + std::to_string(b->device) + ")");
    if (flags != 0) return fail(a, GK_E_ARG, "gk_join: unknown flag bits (flags = " + std::to_string(flags) + ")");
    for (gk_ctx *c : {a, b}) {
        const char *side = c == a ? "a" : "b";
        if (!c->sba) return fail(a, GK_E_STATE, std::string("gk_join: no sequence loaded in context ") + side);
        if (!c->have_starts || !c->sorted)
            return fail(a, GK_E_STATE, std::string("gk_join: the k-mers of context ") + side +
                                           " are not sorted: call gk_sort first");
    }
    if (a->sort_len != b->sort_len)
        return fail(a, GK_E_ARG, "gk_join: the sort lengths differ (a: " + std::to_string(a->sort_len) +
                                     ", b: " + std::to_string(b->sort_len) + ")");
    if (a->canonical != b->canonical)
        return fail(a, GK_E_ARG, std::string("gk_join: one side is sorted by canonical k-mers and the other is not (a: ") +
                                     (a->canonical ? "canonical" : "forward") + ", b: " +
                                     (b->canonical ? "canonical" : "forward") + ")");
    if (a->sort_len == 0)
        return fail(a, GK_E_UNSUPPORTED, "gk_join: the contexts are sorted with max_kmer_len None (sort length 0); "
                                         "a join needs one fixed length");
    for (gk_ctx *c : {a, b})
        if (c->min_k != c->sort_len)
            return fail(a, GK_E_UNSUPPORTED,
                        std::string("gk_join: context ") + (c == a ? "a" : "b") + " holds k-mers cut short by a contig end "
                            "(min_kmer_len = " + std::to_string(c->min_k) + ", sort length = " +
                            std::to_string(c->sort_len) + ")");
    GK_TRY_HIP(a, hipSetDevice(a->device));

    // B first, on its own stream, and complete before A's stream reads its buffers
    if (int rc = join_unique(b)) return b == a ? rc : fail(a, rc, std::string("gk_join: context b: ") + b->err);
    if (int rc = materialize_starts(b)) return b == a ? rc : fail(a, rc, std::string("gk_join: context b: ") + b->err);
    GK_TRY_HIP(a, hipStreamSynchronize(b->stream));
    if (int rc = join_unique(a)) return rc;
    if (int rc = materialize_starts(a)) return rc;
    const uint64_t na = a->n_unique, nb = b->n_unique;

    // path: the merge of the keys when both sides hold final 2-bit keys of one layout, else the bytes
    const bool keys_ok = lookup_keys_usable(a) && lookup_keys_usable(b) && a->spec.symbols == b->spec.symbols;
    bool use_keys = keys_ok;
    const int path = query::parse_path(opt("GKM_JOIN_PATH"));
    if (path < 0) return fail(a, GK_E_ARG, "GKM_JOIN_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !keys_ok)
        return fail(a, GK_E_UNSUPPORTED,
                    "GKM_JOIN_PATH=keys: the contexts do not both hold final one-word 2-bit forward keys");
    if (path == query::kPathBytes) use_keys = false;

    uint32_t *d_first, *d_count;
    unsigned long long *d_sums;
    GK_TRY_HIP(a, scratch(a, "join_first", na, &d_first));
    GK_TRY_HIP(a, scratch(a, "join_count", na, &d_count));
    GK_TRY_HIP(a, scratch(a, "join_sums", (uint64_t)4, &d_sums));
    GK_TRY_HIP(a, hipMemsetAsync(d_sums, 0, 4 * sizeof *d_sums, a->stream));
    if (na > 0 && nb == 0) {  // nothing of A is in an empty B: insertion point 0
        GK_TRY_HIP(a, hipMemsetAsync(d_first, 0, 4 * na, a->stream));
        GK_TRY_HIP(a, hipMemsetAsync(d_count, 0, 4 * na, a->stream));
    } else if (na > 0 && use_keys) {
        const uint64_t tiles = join::tile_count(na, nb);
        uint32_t *splits;
        GK_TRY_HIP(a, scratch(a, "join_splits", tiles + 1, &splits));
        const uint64_t *ka = a->keys[a->cur], *kb = b->keys[b->cur];
        int slot;
        timer_begin(a, "join_partition", &slot);
        timer_units(a, slot, tiles + 1);
        hipLaunchKernelGGL(join_partition_kernel, dim3(join_grid((tiles + kJoinThreads) / kJoinThreads)),
                           dim3(kJoinThreads), 0, a->stream, ka, a->idx_b, na, kb, b->idx_b, nb, tiles, splits);
        GK_TRY_HIP(a, hipGetLastError());
        timer_end(a, slot);
        timer_begin(a, "join_keys", &slot);
        timer_units(a, slot, na + nb);
        hipLaunchKernelGGL(join_keys_kernel, dim3(join_grid(tiles)), dim3(kJoinThreads), 0, a->stream, ka, a->idx_b,
                           a->ucount, na, kb, b->idx_b, b->ucount, nb, b->n, tiles, splits, d_first, d_count, d_sums);
        GK_TRY_HIP(a, hipGetLastError());
        timer_end(a, slot);
    } else if (na > 0) {
        const dim3 grid(join_grid((na + kJoinThreads - 1) / kJoinThreads)), block(kJoinThreads);
        int slot;
        timer_begin(a, "join_bytes", &slot);
        timer_units(a, slot, na);
        if (a->canonical)
            hipLaunchKernelGGL((join_bytes_kernel<true>), grid, block, 0, a->stream, a->sba, a->vals[a->cur], a->idx_b,
                               a->ucount, na, b->sba, b->vals[b->cur], b->n, (int)a->sort_len, d_first, d_count, d_sums);
        else
            hipLaunchKernelGGL((join_bytes_kernel<false>), grid, block, 0, a->stream, a->sba, a->vals[a->cur], a->idx_b,
                               a->ucount, na, b->sba, b->vals[b->cur], b->n, (int)a->sort_len, d_first, d_count, d_sums);
        GK_TRY_HIP(a, hipGetLastError());
        timer_end(a, slot);
    }
    uint64_t sums[4] = {0, 0, 0, 0};
    GK_TRY_HIP(a, read_back(a, d_sums, sizeof sums, sums));  // (synchronises a's stream)
    a->join_n = na;
    a->join_valid = true;
    if (stats) {
        stats->n_distinct_a = na;
        stats->n_distinct_b = nb;
        stats->n_shared = sums[0];
        stats->occ_a_shared = sums[1];
        stats->occ_b_shared = sums[2];
        stats->occ_min = sums[3];
    }
    return GK_OK;
}

extern "C" int gk_copy_join(gk_ctx *c, uint64_t *b_first, uint32_t *b_count, uint64_t n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!join_is_valid(c)) return fail(c, GK_E_STATE, "call gk_join first");
    if (n != c->join_n)
        return fail(c, GK_E_ARG, "n (" + std::to_string(n) + ") differs from the distinct k-mer count (" +
                                     std::to_string(c->join_n) + ")");
    if (n == 0) return GK_OK;
    uint32_t *d_first, *d_count;
    GK_TRY_HIP(c, scratch(c, "join_first", n, &d_first));
    GK_TRY_HIP(c, scratch(c, "join_count", n, &d_count));
    if (b_count) GK_TRY_HIP(c, hipMemcpyAsync(b_count, d_count, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (b_first) {  // widened on the way out, as gk_copy_unique's group starts
        std::vector<uint32_t> tmp(n);
        GK_TRY_HIP(c, hipMemcpyAsync(tmp.data(), d_first, 4 * n, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < n; ++i) b_first[i] = tmp[i];
    }
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_device_join(gk_ctx *c, void **b_first, void **b_count, uint64_t *n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!join_is_valid(c)) return fail(c, GK_E_STATE, "call gk_join first");
    uint32_t *d_first, *d_count;
    GK_TRY_HIP(c, scratch(c, "join_first", c->join_n, &d_first));
    GK_TRY_HIP(c, scratch(c, "join_count", c->join_n, &d_count));
    if (b_first) *b_first = d_first;
    if (b_count) *b_count = d_count;
    if (n) *n = c->join_n;
    return GK_OK;
}

extern "C" int gk_join_mask(gk_ctx *c, int keep) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (keep != GK_JOIN_KEEP_ABSENT && keep != GK_JOIN_KEEP_PRESENT)
        return fail(c, GK_E_ARG, "gk_join_mask: keep (" + std::to_string(keep) +
                                     ") must be GK_JOIN_KEEP_ABSENT (1) or GK_JOIN_KEEP_PRESENT (2)");
    if (!join_is_valid(c)) return fail(c, GK_E_STATE, "call gk_join first");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    const uint64_t n = c->n;
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->mask), &c->mask_cap, n + 64));
    c->mask_n = n;
    if (n == 0) return GK_OK;
    uint32_t *d_count;
    GK_TRY_HIP(c, scratch(c, "join_count", c->join_n, &d_count));
    int slot;
    timer_begin(c, "join_mask", &slot);
    timer_units(c, slot, n);
    hipLaunchKernelGGL(join_mask_kernel, dim3(join_grid((n + kJoinMaskTile - 1) / kJoinMaskTile)), dim3(kJoinThreads), 0,
                       c->stream, c->idx_b, d_count, c->join_n, n, keep == GK_JOIN_KEEP_PRESENT ? 1 : 0, c->mask);
    GK_TRY_HIP(c, hipGetLastError());
    timer_end(c, slot);
    return GK_OK;
}
