// gkm_doubling.hip -- gk_sort by prefix doubling: max_kmer_len None (suffix order up to
// '$', the Kmers default) or a bound too long for direct keys.  Every position of the sequence is
// ranked: seed keys of 29 (ACGT, 2 bits + length) / 16 (IUPAC) symbols, then rounds that double the
// symbols compared -- over the groups still tied (large arrays, msd_sort_groups) or over the whole
// array by (rank[p], rank[p + h]) pairs, each a stable radix sort -- and finally the starts with
// >= min_kmer_len bases are kept, in order.
#include <algorithm>

#include "gkm_internal.h"

namespace gkm {

// ---------------------------------------------------------------------------------------------
// prefix-doubling kernels
// ---------------------------------------------------------------------------------------------

// R[vals[i]] = gstart[gid[i] - 1] + 1   (rank = 1 + index of the group's first element)
__global__ __launch_bounds__(256) void rank_scatter_kernel(const uint32_t *__restrict__ vals,
                                                           const uint32_t *__restrict__ gid,
                                                           const uint32_t *__restrict__ gstart, uint64_t n,
                                                           uint32_t *__restrict__ R) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        R[vals[i]] = gstart[gid[i] - 1] + 1;
}

// Groups of the current order that may still split: more than one member, and members longer than
// the h symbols the keys hold.  Members of a group share their first h symbols, so a group whose
// first member's suffix (to '$' / the end) is shorter than h holds equal k-mers and is final --
// the '$'-terminated tails shared by several contigs, which no doubling round can separate.  A
// suffix of exactly h symbols decides nothing: the keys carry no '$' behind the h-th symbol (the
// ACGT length field stops at h), so the other members may go on, and differ, behind it.
__global__ __launch_bounds__(256) void unresolved_groups_kernel(const uint32_t *__restrict__ vals,
                                                                const uint32_t *__restrict__ gstart, uint64_t G,
                                                                uint64_t n, const uint32_t *__restrict__ seg,
                                                                uint32_t nseg, uint64_t L, uint64_t h,
                                                                uint32_t *__restrict__ count) {
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < G; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = gstart[g], e = g + 1 < G ? gstart[g + 1] : n;
        if (e - b < 2) continue;
        const uint64_t p = vals[b];
        if (seg_end_of(seg, nseg, L, p) - p + 1 >= h) atomicAdd(count, 1u);
    }
}

// key = rank[p] << 32 | (p + o <= seg_end(p) ? rank[p + o] : 0)
__global__ __launch_bounds__(256) void pair_keys_kernel(const uint32_t *__restrict__ vals,
                                                        const uint32_t *__restrict__ R,
                                                        const uint32_t *__restrict__ seg, uint32_t nseg, uint64_t L,
                                                        uint64_t o, uint64_t n, int bw,
                                                        uint64_t *__restrict__ keys) {
    // (rank of p, rank of p + o) in 2 bw bits: ranks are <= n < 2^bw
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = vals[i];
        const uint64_t q = p + o;
        const uint32_t r2 = (q <= seg_end_of(seg, nseg, L, p)) ? R[q] : 0u;
        keys[i] = ((uint64_t)R[p] << bw) | r2;
    }
}

// Prefix doubling by tied groups (rounds_by_groups): the rank of p + o for the elements
// still tied (flags: 1 starts a group), the others untouched
__global__ __launch_bounds__(256) void member_r2_kernel(const uint8_t *__restrict__ flags,
                                                        const uint32_t *__restrict__ vals,
                                                        const uint32_t *__restrict__ R,
                                                        const uint32_t *__restrict__ seg, uint32_t nseg, uint64_t L,
                                                        uint64_t o, uint64_t n, uint64_t *__restrict__ keys) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (flags[i] != 0 && (i + 1 >= n || flags[i + 1] != 0)) continue;  // a group of one: final
        const uint64_t p = vals[i];
        const uint64_t q = p + o;
        keys[i] = (q <= seg_end_of(seg, nseg, L, p)) ? R[q] : 0u;
    }
}

// the groups after a round: a group start stays one, a tied element starts a group where the
// round's sort found its key different from its predecessor's (heads of the sorted groups)
__global__ __launch_bounds__(256) void merge_heads_kernel(const uint8_t *__restrict__ fold,
                                                          const uint8_t *__restrict__ heads, uint64_t n,
                                                          uint8_t *__restrict__ fnew) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        fnew[i] = (fold[i] != 0 || heads[i] != 0) ? 1 : 0;
}

// new ranks (group start + 1) of the elements that were tied before the round; the others keep theirs
__global__ __launch_bounds__(256) void member_rank_kernel(const uint8_t *__restrict__ fold,
                                                          const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ gid,
                                                          const uint32_t *__restrict__ gstart, uint64_t n,
                                                          uint32_t *__restrict__ R) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (fold[i] != 0 && (i + 1 >= n || fold[i + 1] != 0)) continue;
        R[vals[i]] = gstart[gid[i] - 1] + 1;
    }
}

// keep starts with >= m bases before the end of their segment
__global__ __launch_bounds__(256) void len_flags_kernel(const uint32_t *__restrict__ vals,
                                                        const uint32_t *__restrict__ seg, uint32_t nseg, uint64_t L,
                                                        uint64_t m, uint64_t n, uint8_t *__restrict__ flags) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = vals[i];
        flags[i] = (p + m - 1 <= seg_end_of(seg, nseg, L, p)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void gather_pairs_kernel(const uint32_t *__restrict__ idx, uint64_t count,
                                                           const uint32_t *__restrict__ vin,
                                                           const uint64_t *__restrict__ kin,
                                                           uint32_t *__restrict__ vout, uint64_t *__restrict__ kout) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        vout[i] = vin[j];
        kout[i] = kin[j];
    }
}

// keys[i] = R[starts[i]] (final rank of a user-provided start)
__global__ __launch_bounds__(256) void rank_gather_kernel(const uint32_t *__restrict__ starts,
                                                          const uint32_t *__restrict__ R, uint64_t n,
                                                          uint64_t *__restrict__ keys) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keys[i] = R[starts[i]];
}

__global__ __launch_bounds__(256) void u32_to_key_kernel(const uint32_t *__restrict__ v, uint64_t n,
                                                         uint64_t *__restrict__ keys) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keys[i] = v[i];
}

__global__ __launch_bounds__(256) void full_key_heads_kernel(const uint64_t *__restrict__ keys, uint64_t n,
                                                             uint8_t *__restrict__ head) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// stable pre-sort of arbitrary start indices by value, so ties end in start order
int presort_by_start(gk_ctx *c) {
    hipLaunchKernelGGL(u32_to_key_kernel, dim3(grid_of(c->n)), dim3(256), 0, c->stream, c->vals[c->cur], c->n,
                       c->keys[c->cur]);
    GK_TRY_HIP(c, hipGetLastError());
    return radix_sort(c, 1, 32, false);
}

// ---------------------------------------------------------------------------------------------
// the steps both kinds of round share (n1: the positions ranked; groups: flags with 1 at a group's
// first element, their starts in idx_b, each element's group number in idx_a)
// ---------------------------------------------------------------------------------------------

// the groups of `flags`: their starts (*G of them) and -- scan -- every element's group number
static int number_groups(gk_ctx *c, const uint8_t *flags, uint64_t n1, uint64_t *G, bool scan) {
    GK_TRY_HIP(c, select_flags(c, flags, n1, c->idx_b, G));
    if (scan) GK_TRY_HIP(c, scan_flags_inclusive(c, flags, n1, c->idx_a));
    return GK_OK;
}

// the groups of equal keys[cur] (sorted), flagged in `flags`
static int group_equal_keys(gk_ctx *c, uint8_t *flags, uint64_t n1, uint64_t *G, bool scan) {
    hipLaunchKernelGGL(full_key_heads_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, c->keys[c->cur], n1, flags);
    GK_TRY_HIP(c, hipGetLastError());
    return number_groups(c, flags, n1, G, scan);
}

// rank every position by the numbered groups of the order `vals`: group start + 1 (0: not a position)
static int rank_positions(gk_ctx *c, const uint32_t *vals, uint64_t n1) {
    GK_TRY_HIP(c, hipMemsetAsync(c->ranks, 0, 4 * (c->sba_len + 64), c->stream));
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, vals, c->idx_a, c->idx_b, n1,
                       c->ranks);
    GK_TRY_HIP(c, hipGetLastError());
    return GK_OK;
}

// whether the order of `vals` by h symbols, in G groups, can still change (M: the bound, 0 = none)
static int order_is_open(gk_ctx *c, const uint32_t *vals, uint64_t G, uint64_t n1, uint64_t h, uint32_t M,
                         bool *open) {
    *open = false;
    if (G == n1) return GK_OK;                       // all distinct
    if (M == 0 && h >= c->max_seg_len) return GK_OK;  // every suffix ends within h symbols
    // every tied group already holds equal k-mers (shared contig tails): done
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(c->scalars + 20), cnt = 0;
    GK_TRY_HIP(c, hipMemsetAsync(d_cnt, 0, 4, c->stream));
    hipLaunchKernelGGL(unresolved_groups_kernel, dim3(grid_of(G)), dim3(256), 0, c->stream, vals, c->idx_b, G, n1,
                       c->seg, (uint32_t)c->nseg, c->sba_len, h, d_cnt);
    GK_TRY_HIP(c, hipGetLastError());
    GK_TRY_HIP(c, hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    *open = cnt != 0;
    return GK_OK;
}

// symbols the next round adds to the h compared so far: it doubles them, up to the bound
static uint64_t next_step(uint64_t h, uint32_t M) { return M ? std::min<uint64_t>(h, M - h) : h; }

// ranks: group start + 1 <= n1 (0: past the segment's end)
static int rank_bits(uint64_t n1) { return std::max(1, bit_width(n1)); }

// ---------------------------------------------------------------------------------------------
// seed, rounds, finishes
// ---------------------------------------------------------------------------------------------

// Seed keys of every position, sorted: ACGT data as 29 symbols of 2 bits + a 5-bit length field (the
// (padded, length) keys of the bounded sort: the same order as '$'-terminated 3-bit codes, 29
// symbols instead of 21, and every key bit carries information for the MSD levels); other data as
// 16 symbols of 4 bits
static int seed_sort(gk_ctx *c, uint64_t n1, KeySpec *seed) {
    *seed = c->acgt ? key_spec(2, 29, bit_width(29), 1) : key_spec(4, 16, 0, 1);
    int slot;
    timer_begin(c, "encode", &slot);
    timer_units(c, slot, n1);
    const bool seed_hist = !sort_keys_msd(c, n1, 1, seed->total_bits);
    GK_TRY_HIP(c, launch_encode_positions(c, *seed, c->keys[0], c->vals[0], seed_hist ? c->hist : nullptr));
    timer_end(c, slot);
    return sort_keys(c, 1, seed->total_bits, seed_hist);
}

// Rounds that sort only the groups still tied (keys[0] / vals[0]; msd_sort_groups), then the keys:
// flags of the current groups (fa), the next round's (fb); ranks of every position in R from the
// second round on (scattered once, then only for the elements a round re-sorts)
static int rounds_by_groups(gk_ctx *c, const KeySpec &seed, uint32_t M, uint64_t n1) {
    const uint64_t L = c->sba_len;
    uint64_t h = (uint64_t)seed.symbols, G = 0;
    uint8_t *fa = c->flags, *fb;
    GK_TRY_HIP(c, scratch(c, "dbl_flags", n1 + 64, &fb));
    if (int rc = group_equal_keys(c, fa, n1, &G, true)) return rc;
    bool ranks_ready = false;  // every position ranked (from the second round on)
    for (int round = 0; !(M && h >= M); ++round) {
        bool open;
        if (int rc = order_is_open(c, c->vals[0], G, n1, h, M, &open)) return rc;
        if (!open) break;
        const uint64_t o = next_step(h, M);
        int bkey = rank_bits(n1);
        if (round == 0) {
            // the rank of p + o after the seed sort (h = seed.symbols) orders like the seed key
            // of p + o, whatever o is: the tied elements read it from their windows, and no
            // position needs ranking yet
            GK_TRY_HIP(c, launch_member_seed_keys(c, seed, fa, c->vals[0], o, n1, c->keys[0]));
            bkey = seed.total_bits;
        } else {
            if (!ranks_ready) {  // every position ranked by the order so far, once
                if (int rc = rank_positions(c, c->vals[0], n1)) return rc;
                ranks_ready = true;
            }
            hipLaunchKernelGGL(member_r2_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, fa, c->vals[0],
                               c->ranks, c->seg, (uint32_t)c->nseg, L, o, n1, c->keys[0]);
            GK_TRY_HIP(c, hipGetLastError());
        }
        if (int rc = msd_sort_groups(c, fa, bkey)) return rc;
        hipLaunchKernelGGL(merge_heads_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, fa, c->heads, n1, fb);
        GK_TRY_HIP(c, hipGetLastError());
        if (int rc = number_groups(c, fb, n1, &G, true)) return rc;
        if (ranks_ready) {  // (else ranked from the current order when a round needs it)
            hipLaunchKernelGGL(member_rank_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, fa, c->vals[0],
                               c->idx_a, c->idx_b, n1, c->ranks);
            GK_TRY_HIP(c, hipGetLastError());
        }
        std::swap(fa, fb);
        h += o;
    }
    // the keys: dense group numbers (equal iff the k-mers are equal, ascending with the order)
    hipLaunchKernelGGL(u32_to_key_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, c->idx_a, n1, c->keys[0]);
    GK_TRY_HIP(c, hipGetLastError());
    return GK_OK;
}

// Rounds that re-sort the whole array by (rank[p], rank[p + o]) pairs (small arrays: LSD)
static int rounds_whole_array(gk_ctx *c, uint64_t h, uint32_t M, uint64_t n1) {
    while (!(M && h >= M)) {
        uint64_t G = 0;
        bool open;
        if (int rc = group_equal_keys(c, c->flags, n1, &G, false)) return rc;
        if (int rc = order_is_open(c, c->vals[c->cur], G, n1, h, M, &open)) return rc;
        if (!open) break;
        GK_TRY_HIP(c, scan_flags_inclusive(c, c->flags, n1, c->idx_a));
        if (int rc = rank_positions(c, c->vals[c->cur], n1)) return rc;
        const uint64_t o = next_step(h, M);
        const int bw = rank_bits(n1);
        hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, c->vals[c->cur], c->ranks,
                           c->seg, (uint32_t)c->nseg, c->sba_len, o, n1, bw, c->keys[c->cur]);
        GK_TRY_HIP(c, hipGetLastError());
        if (int rc = sort_keys(c, 1, 2 * bw, false)) return rc;
        h += o;
    }
    return GK_OK;
}

// finish: the enumerated starts with >= m bases, in order, into the other buffers
static int keep_long_enough(gk_ctx *c, uint32_t m, uint64_t n1, uint64_t n_kmers) {
    hipLaunchKernelGGL(len_flags_kernel, dim3(grid_of(n1)), dim3(256), 0, c->stream, c->vals[c->cur], c->seg,
                       (uint32_t)c->nseg, c->sba_len, (uint64_t)m, n1, c->flags);
    GK_TRY_HIP(c, hipGetLastError());
    uint64_t cnt = 0;
    GK_TRY_HIP(c, select_flags(c, c->flags, n1, c->idx_a, &cnt));
    if (cnt != n_kmers) return fail(c, GK_E_HIP, "doubling: k-mer count mismatch after filtering");
    const int o = c->cur ^ 1;
    hipLaunchKernelGGL(gather_pairs_kernel, dim3(grid_of(cnt)), dim3(256), 0, c->stream, c->idx_a, cnt,
                       c->vals[c->cur], c->keys[c->cur], c->vals[o], c->keys[o]);
    GK_TRY_HIP(c, hipGetLastError());
    c->cur = o;
    c->n = cnt;
    return GK_OK;
}

// finish: the final dense rank of every position, then the user's starts (the side buffer `user`,
// freed here) sorted by it
static int sort_user_starts(gk_ctx *c, uint32_t *user, uint64_t n_kmers, uint64_t n1) {
    uint64_t G = 0;
    if (int rc = group_equal_keys(c, c->flags, n1, &G, true)) return rc;
    if (int rc = rank_positions(c, c->vals[c->cur], n1)) return rc;
    c->n = n_kmers;
    c->cur = 0;
    if (n_kmers) GK_TRY_HIP(c, hipMemcpyAsync(c->vals[0], user, 4 * n_kmers, hipMemcpyDeviceToDevice, c->stream));
    if (int rc = presort_by_start(c)) return rc;
    hipLaunchKernelGGL(rank_gather_kernel, dim3(grid_of(n_kmers)), dim3(256), 0, c->stream, c->vals[c->cur],
                       c->ranks, n_kmers, c->keys[c->cur]);
    GK_TRY_HIP(c, hipGetLastError());
    if (int rc = radix_sort(c, 1, 32, false)) return rc;
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(user);
    return GK_OK;
}

// Prefix doubling over all non-'$' positions; M = 0 means unbounded (suffix order).
int sort_doubling(gk_ctx *c, uint32_t M) {
    const uint64_t n_kmers = c->n;
    const bool was_enumerated = c->enumerated;
    const uint32_t m = c->min_k;
    uint32_t *user = nullptr;  // user-provided starts survive in a side buffer
    if (!was_enumerated && n_kmers > 0) {
        GK_TRY_HIP(c, hipMalloc(&user, 4 * n_kmers));
        GK_TRY_HIP(c, hipMemcpyAsync(user, c->vals[c->cur], 4 * n_kmers, hipMemcpyDeviceToDevice, c->stream));
    }
    // universe: every position inside a segment (min length 1)
    const uint64_t n1 = c->sba_len - (c->nseg - 1);
    int rc = ensure_elems(c, std::max(n1, n_kmers), 1);
    if (rc != GK_OK) return rc;
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->flags), &c->flags_cap, n1 + 64));
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->idx_a), &c->idx_cap, 4 * (n1 + 64)));
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->idx_b), &c->idx_b_cap, 4 * (n1 + 64)));
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->ranks), &c->ranks_cap, 4 * (c->sba_len + 64)));
    c->n = n1;
    c->cur = 0;
    // large universes: the rounds sort only the groups still tied (MSD, msd_sort_groups); small ones
    // re-sort the whole array by rank pairs each round (LSD)
    const bool by_groups = sort_keys_msd(c, n1, 1, 64);
    KeySpec seed;
    if ((rc = seed_sort(c, n1, &seed))) return rc;
    // (a bound within the seed's symbols leaves no round: the direct path covers it; kept for safety)
    rc = by_groups && c->cur == 0 ? rounds_by_groups(c, seed, M, n1)
                                  : rounds_whole_array(c, (uint64_t)seed.symbols, M, n1);
    if (rc != GK_OK) return rc;

    if (was_enumerated && n_kmers == n1) {
        // every position of the universe has >= m bases (m = 1, or no shorter tails): the order is
        // already the k-mers' order, in place
        c->n = n1;
    } else if (was_enumerated) {
        if ((rc = keep_long_enough(c, m, n1, n_kmers))) return rc;
    } else {
        if ((rc = sort_user_starts(c, user, n_kmers, n1))) return rc;
    }
    // (the keys are ranks: only their order means anything)
    sort_finished(c, KeySpec{0, 0, 0, (int)m, 1, 64}, M, /*canonical*/ false, /*keys_stale*/ false, /*keys_are_ranks*/ true);
    return GK_OK;
}

}  // namespace gkm
