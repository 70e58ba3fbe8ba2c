// gkm_msd_lists.h -- the bucket lists between the stages of the MSD sort: the list counters and
// sums, the Lists struct and the routing of a sub-bucket by size (route, classify_kernel), the
// expansion of packed and compact level outputs, uniform buckets and the done copy.
// Private to gkm_msd.hip.  Needs gkm_msd_config.h and gkm_msd_scan.h (tiles_of, chunks_of).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkm_msd_config.h"
#include "gkm_msd_scan.h"
#include "gkm_partition.h"

namespace gkm {

// wave-aggregated append of one entry per flagged lane; returns the entry index
__device__ __forceinline__ uint32_t wave_append(bool flag, uint32_t *counter, int lane) {
    const uint64_t m = __ballot(flag);
    if (!m) return 0;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    return base + (uint32_t)__popcll(m & lt_mask);
}

// list counters (device, one array): next global level, done, then the local classes
enum { kCtrBig = 0, kCtrDone = 1, kCtrLoc = 2, kLists = kCtrLoc + kLocal, kCtrNbCopy = kLists, kCtrN = 8 + 2 };
// (kCtrNbCopy: the big list's count kept while its counter restarts, MsdDriver::drop_uniform_dev)
// element sums per list, then the next global level's tile and chunk totals (its tile tables'
// sizes, known with the list counts so that planning the level needs no read-back of its own)
enum { kSumTiles = kLists, kSumChunks = kLists + 1, kSumN = kLists + 2 };

struct Lists {
    uint32_t *nb_start, *nb_len;                 // buckets for the next global level
    uint32_t *dn_start, *dn_len;                 // key bits exhausted: final as they stand
    uint8_t *dn_par;
    uint2 *loc[kLocal];                          // local entries by class
    // per entry: the bucket's sorted key bits (its prefix), | kCompact when its elements are
    // stored compact (a compact level's output, see level_pass); null: not recorded
    uint64_t *nb_pref;
    uint64_t *loc_pref[kLocal];
};

// A compact level writes per element, in the key array, the key bits below the next 8-bit digit
// (high half) and the start (low half), and that digit in the digit bytes: 9 B instead of 12 (and
// two stores instead of three); the bucket's prefix completes the key.
constexpr uint64_t kCompact = 1ull << 63;

__device__ __forceinline__ uint64_t compact_key(uint64_t pref, int hi, int B, uint32_t dig, uint32_t low) {
    const int rem = B - hi;  // 9..40
    return ((pref & ~kCompact) << rem) | ((uint64_t)dig << (rem - 8)) | (uint64_t)low;
}

// local class of a bucket of <= kBlockMax elements
__host__ __device__ constexpr uint32_t local_cap(int cls) {
    return cls == 0 ? 256 : cls == 1 ? 512 : cls == 2 ? 1024 : cls == 3 ? 4096 : cls == 5 ? 8192 : kTiny;
}

// list of a live sub-bucket of `size` elements (kCtr* index)
__device__ __forceinline__ int list_of(uint32_t size, int hi, int B, bool allow_big) {
    if (hi >= B) return kCtrDone;
    if (size > (uint32_t)kBlockMax && allow_big) return kCtrBig;
    if (size <= (uint32_t)kTiny) return kCtrLoc + 4;
    return kCtrLoc + (size <= local_cap(0) ? 0 : size <= local_cap(1) ? 1 : size <= local_cap(2) ? 2
                      : size <= local_cap(3) ? 3 : 5);
}

// entry `at` of list l for a sub-bucket
__device__ __forceinline__ void put_entry(const Lists &L, int l, uint32_t at, uint32_t st, uint32_t size, int hi,
                                          int parity, uint64_t pref = 0) {
    // (global stores: flat ones, through pointers read from memory, would make every later
    // memory wait of the kernel a full drain)
    if (l == kCtrBig) {
        gmem(L.nb_start)[at] = st;
        gmem(L.nb_len)[at] = size;
        if (L.nb_pref) gmem(L.nb_pref)[at] = pref;
    } else if (l == kCtrDone) {
        gmem(L.dn_start)[at] = st;
        gmem(L.dn_len)[at] = size;
        gmem(L.dn_par)[at] = (uint8_t)parity;
    } else {
        const uint2 le = local_entry(st, size, hi, parity);
        gmem(reinterpret_cast<uint64_t *>(L.loc[l - kCtrLoc]))[at] = ((uint64_t)le.y << 32) | le.x;
        if (L.loc_pref[l - kCtrLoc]) gmem(L.loc_pref[l - kCtrLoc])[at] = pref;
    }
}

// route one sub-bucket (size >= 1) by size; hi = key bits sorted once it is cut out
__device__ __forceinline__ void route(uint32_t st, uint32_t size, int hi, int B, int parity, bool allow_big,
                                      const Lists &L, uint32_t *ctr, int lane) {
    const int li = size >= 1 ? list_of(size, hi, B, allow_big) : -1;
#pragma unroll
    for (int l = 0; l < kLists; ++l) {
        const uint32_t at = wave_append(li == l, &ctr[l], lane);
        if (li == l) put_entry(L, l, at, st, size, hi, parity);
    }
}

// The sub-buckets of one global level, one per thread: a workgroup-aggregated append (one
// atomic per list per workgroup) into the next-level / done / block-local / wave-local lists;
// sums[l] += elements routed to list l (for the profile's work counts).
constexpr int kClassT = 1024;

// Prefixes: sub-bucket i of a partition by pw-bit digits has parent i >> pw (prefix ppref[i >> pw],
// 0 when null) and digit i & (2^pw - 1); with pw = 0 the entries are whole buckets (prefix ppref[i]).
// compact: the level wrote compact elements (the entries get kCompact).
__global__ __launch_bounds__(kClassT) void classify_kernel(const uint32_t *__restrict__ seg_base,
                                                           const uint32_t *__restrict__ seg_cnt, uint64_t nsub, int hi,
                                                           int B, int parity, Lists L, uint32_t *__restrict__ ctr,
                                                           unsigned long long *__restrict__ sums, uint32_t min_size,
                                                           const uint64_t *__restrict__ ppref, int pw, int compact,
                                                           uint32_t tile, uint32_t ctiles) {
    constexpr int NW = kClassT / 64;
    __shared__ uint32_t s_cnt[kLists][NW];
    __shared__ uint32_t s_elems[kLists][NW];
    __shared__ uint32_t s_base[kLists];
    __shared__ uint32_t s_tc[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kClassT + tid;
    const uint32_t size = i < nsub ? seg_cnt[i] : 0, st = i < nsub ? seg_base[i] : 0;
    const int li = size >= min_size ? list_of(size, hi, B, true) : -1;
    bool f[kLists];
#pragma unroll
    for (int l = 0; l < kLists; ++l) f[l] = li == l;
    uint32_t below[kLists];
#pragma unroll
    for (int l = 0; l < kLists; ++l) {
        const uint64_t m = __ballot(f[l]);
        below[l] = lanes_below(m);
        uint32_t e = f[l] ? size : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off);
        if (lane == 0) {
            s_cnt[l][wave] = (uint32_t)__popcll(m);
            s_elems[l][wave] = e;
        }
    }
    {
        uint32_t tl = li == kCtrBig ? tiles_of(size, tile) : 0, ch = li == kCtrBig ? chunks_of(size, tile, ctiles) : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            tl += __shfl_xor(tl, off);
            ch += __shfl_xor(ch, off);
        }
        if (lane == 0) {
            s_tc[0][wave] = tl;
            s_tc[1][wave] = ch;
        }
    }
    __syncthreads();
    if (tid >= 64 && tid < 66) {  // (another wave than the list totals below)
        unsigned long long t = 0;
        for (int w = 0; w < NW; ++w) t += s_tc[tid - 64][w];
        if (t) atomicAdd(&sums[kSumTiles + tid - 64], t);
    }
    if (tid < kLists) {
        uint32_t tot = 0;
        unsigned long long el = 0;
        for (int w = 0; w < NW; ++w) {
            tot += s_cnt[tid][w];
            el += s_elems[tid][w];
        }
        s_base[tid] = tot ? atomicAdd(&ctr[tid], tot) : 0;
        if (el) atomicAdd(&sums[tid], el);
    }
    __syncthreads();
    uint32_t at[kLists];
#pragma unroll
    for (int l = 0; l < kLists; ++l) {
        uint32_t pre = s_base[l];
        for (int w = 0; w < wave; ++w) pre += s_cnt[l][w];
        at[l] = pre + below[l];
    }
    uint64_t pref = 0;
    if (li >= 0) {
        if (pw > 0) pref = ((ppref ? ppref[i >> pw] & ~kCompact : 0ull) << pw) | (i & ((1ull << pw) - 1));
        else pref = ppref ? ppref[i] & ~kCompact : 0ull;
        if (compact) pref |= kCompact;
    }
#pragma unroll
    for (int l = 0; l < kLists; ++l)
        if (li == l) put_entry(L, l, at[l], st, size, hi, parity, pref);
}

// workgroups per bucket (grid.y) of the per-bucket copy kernels below: the buckets they see are
// few but can be huge (a repeat's group of identical k-mers: 250 K elements at C4), and one
// workgroup walking such a bucket alone took 3 ms per C4 rank
static unsigned bucket_split(uint64_t nbuckets) { return nbuckets <= 4096 ? 32u : nbuckets <= 65536 ? 4u : 1u; }

// (key, start) of packed-pair elements (a MODE 5 level's output, gkm_partition.h) in place, for
// the buckets a packed-pair level's output goes to that do not read pairs: the next level when it
// is not compact, and the local finishing classes.  Bucket j: start bst[j], length blen[j], sorted
// key bits bpref[j] (the top hi of B); gridDim.y workgroups per bucket.
__global__ __launch_bounds__(256) void expand_pair_kernel(const uint32_t *__restrict__ bst,
                                                          const uint32_t *__restrict__ blen,
                                                          const uint64_t *__restrict__ bpref, int hi, int B, int shi,
                                                          uint64_t *__restrict__ kio, const uint16_t *__restrict__ in16,
                                                          uint32_t *__restrict__ vout) {
    const uint64_t st = bst[blockIdx.x];
    const uint32_t len = blen[blockIdx.x];
    const uint64_t top = (bpref[blockIdx.x] & ~kCompact) << (B - hi);
    for (uint32_t e = blockIdx.y * 256 + threadIdx.x; e < len; e += gridDim.y * 256) {
        uint64_t key;
        uint32_t val;
        unpack_pair(kio[st + e], in16[st + e], shi, key, val);
        kio[st + e] = top | key;
        vout[st + e] = val;
    }
}

// the same over local-list entries [first, first + count) (entry: start, len << 8 | hi << 1 | parity;
// prefixes in pref[]) -- the local buckets a packed-pair level's classify listed
__global__ __launch_bounds__(256) void expand_pair_list_kernel(const uint2 *__restrict__ list,
                                                               const uint64_t *__restrict__ pref, uint32_t first,
                                                               int B, int shi, uint64_t *__restrict__ kio,
                                                               const uint16_t *__restrict__ in16,
                                                               uint32_t *__restrict__ vout) {
    const uint2 en = list[first + blockIdx.x];
    const uint64_t st = en.x;
    const uint32_t len = en.y >> 8;
    const int hi = (en.y >> 1) & 127;
    const uint64_t top = (pref[first + blockIdx.x] & ~kCompact) << (B - hi);
    for (uint32_t e = threadIdx.x; e < len; e += 256) {
        uint64_t key;
        uint32_t val;
        unpack_pair(kio[st + e], in16[st + e], shi, key, val);
        kio[st + e] = top | key;
        vout[st + e] = val;
    }
}

// packed-L0 elements (P88: the digit byte above a packed pair) -> (key bits below the sorted ones,
// start)
__device__ __forceinline__ void unpack_p88(uint64_t a, uint32_t lo, uint32_t dg, int shi, uint64_t &rel, uint32_t &val) {
    unpack_pair(a, lo, shi, rel, val);
    rel |= (uint64_t)dg << (64 - shi);
}

// (key, start) of packed-L0 elements in place, for the buckets whose next reader does not take the
// packed form: the big buckets when the level behind the L0 writes no packed pairs itself (gridDim.y
// workgroups per bucket), and the local classes' entries (expand_p88_list_kernel)
__global__ __launch_bounds__(256) void expand_p88_kernel(const uint32_t *__restrict__ bst,
                                                         const uint32_t *__restrict__ blen,
                                                         const uint64_t *__restrict__ bpref, int hi, int B, int shi,
                                                         uint64_t *__restrict__ kio, const uint16_t *__restrict__ in16,
                                                         const uint8_t *__restrict__ in8, uint32_t *__restrict__ vout) {
    const uint64_t st = bst[blockIdx.x];
    const uint32_t len = blen[blockIdx.x];
    const uint64_t top = (bpref[blockIdx.x] & ~kCompact) << (B - hi);
    for (uint32_t e = blockIdx.y * 256 + threadIdx.x; e < len; e += gridDim.y * 256) {
        uint64_t rel;
        uint32_t val;
        unpack_p88(kio[st + e], in16[st + e], in8[st + e], shi, rel, val);
        kio[st + e] = top | rel;
        vout[st + e] = val;
    }
}

__global__ __launch_bounds__(256) void expand_p88_list_kernel(const uint2 *__restrict__ list,
                                                              const uint64_t *__restrict__ pref, int B, int shi,
                                                              uint64_t *__restrict__ kio, const uint16_t *__restrict__ in16,
                                                              const uint8_t *__restrict__ in8,
                                                              uint32_t *__restrict__ vout) {
    const uint2 en = list[blockIdx.x];
    const uint64_t st = en.x;
    const uint32_t len = en.y >> 8;
    const int hi = (en.y >> 1) & 127;
    const uint64_t top = (pref[blockIdx.x] & ~kCompact) << (B - hi);
    for (uint32_t e = threadIdx.x; e < len; e += 256) {
        uint64_t rel;
        uint32_t val;
        unpack_p88(kio[st + e], in16[st + e], in8[st + e], shi, rel, val);
        kio[st + e] = top | rel;
        vout[st + e] = val;
    }
}

// the same over pieces (first_level_from_pieces: the prefetched L0's region buckets): piece j at
// pp[j], pp[np + j] elements, its bucket (the top hi key bits) pp[2 np + j]
__global__ __launch_bounds__(256) void expand_p88_pieces_kernel(const uint64_t *__restrict__ pp, uint32_t np, int hi,
                                                                int B, int shi, uint64_t *__restrict__ kio,
                                                                const uint16_t *__restrict__ in16,
                                                                const uint8_t *__restrict__ in8,
                                                                uint32_t *__restrict__ vout) {
    const uint64_t st = pp[blockIdx.x], len = pp[np + blockIdx.x];
    const uint64_t top = pp[2 * (uint64_t)np + blockIdx.x] << (B - hi);
    for (uint64_t e = blockIdx.y * 256 + threadIdx.x; e < len; e += gridDim.y * 256) {
        uint64_t rel;
        uint32_t val;
        unpack_p88(kio[st + e], in16[st + e], in8[st + e], shi, rel, val);
        kio[st + e] = top | rel;
        vout[st + e] = val;
    }
}

// keys of compact elements (gridDim.y workgroups per bucket): prefix | digit | low bits
__global__ __launch_bounds__(256) void expand_compact_kernel(const uint32_t *__restrict__ bst,
                                                             const uint32_t *__restrict__ blen,
                                                             const uint64_t *__restrict__ bpref, int hi, int B,
                                                             const uint8_t *__restrict__ nd,
                                                             uint64_t *__restrict__ kio, uint32_t *__restrict__ vout,
                                                             const uint32_t *__restrict__ nb_dev = nullptr) {
    if (nb_dev && blockIdx.x >= *nb_dev) return;  // (a grid sized by a bound: the count is on the device)
    const uint64_t st = bst[blockIdx.x];
    const uint32_t len = blen[blockIdx.x];
    const uint64_t pf = bpref[blockIdx.x];
    for (uint32_t e = blockIdx.y * 256 + threadIdx.x; e < len; e += gridDim.y * 256) {
        const uint64_t x = kio[st + e];
        kio[st + e] = compact_key(pf, hi, B, nd[st + e], (uint32_t)(x >> 32));
        vout[st + e] = (uint32_t)x;
    }
}

// one round's lists, copied to device memory for the wave kernels
__global__ void lists_store_kernel(Lists L, Lists *__restrict__ dst) { *dst = L; }

// Next-level buckets whose keys are all equal (a repeat's group of identical k-mers: 250 K
// elements of (CA)n at C4) would go through every remaining global level without splitting, each
// with its host round trips.  uniform_flag_kernel marks the buckets holding two different keys
// (gridDim.y workgroups per bucket); route_uniform_kernel sends the others to the done list.
__global__ __launch_bounds__(256) void uniform_flag_kernel(const uint32_t *__restrict__ bst,
                                                           const uint32_t *__restrict__ blen,
                                                           const uint64_t *__restrict__ keys,
                                                           uint32_t *__restrict__ mixed,
                                                           const uint32_t *__restrict__ nb_dev = nullptr,
                                                           uint32_t *__restrict__ nb_copy = nullptr) {
    if (nb_copy && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nb_copy = *nb_dev;
    if (nb_dev && blockIdx.x >= *nb_dev) return;
    const uint64_t st = bst[blockIdx.x];
    const uint32_t len = blen[blockIdx.x];
    const uint64_t k0 = keys[st];
    uint64_t acc = 0;
    for (uint32_t e = blockIdx.y * 256 + threadIdx.x; e < len; e += gridDim.y * 256) acc |= keys[st + e] ^ k0;
    if (__syncthreads_or(acc != 0) && threadIdx.x == 0) atomicOr(&mixed[blockIdx.x], 1u);
}

__global__ __launch_bounds__(256) void route_uniform_kernel(const uint32_t *__restrict__ bst,
                                                            const uint32_t *__restrict__ blen,
                                                            const uint64_t *__restrict__ bpref, uint32_t nb,
                                                            const uint32_t *__restrict__ mixed, Lists L, int parity,
                                                            uint32_t *__restrict__ ctr,
                                                            unsigned long long *__restrict__ sums, uint32_t tile,
                                                            uint32_t ctiles, const uint32_t *__restrict__ nb_dev = nullptr) {
    if (nb_dev) nb = *nb_dev;
    for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < nb; b += gridDim.x * 256) {
        if (mixed[b]) {
            const uint32_t at = atomicAdd(&ctr[kCtrBig], 1u);
            put_entry(L, kCtrBig, at, bst[b], blen[b], 0, parity, bpref ? bpref[b] : 0);
            atomicAdd(&sums[kCtrBig], (unsigned long long)blen[b]);
            atomicAdd(&sums[kSumTiles], (unsigned long long)tiles_of(blen[b], tile));
            atomicAdd(&sums[kSumChunks], (unsigned long long)chunks_of(blen[b], tile, ctiles));
        } else {
            put_entry(L, kCtrDone, atomicAdd(&ctr[kCtrDone], 1u), bst[b], blen[b], 0, parity);
        }
    }
}

// sub-buckets whose key bits are exhausted: in order already (copied to buffer 0 if needed);
// all keys equal, so the only head is the first element (gridDim.y workgroups per bucket)
__global__ __launch_bounds__(256) void done_copy_kernel(const uint32_t *__restrict__ dn_start,
                                                        const uint32_t *__restrict__ dn_len,
                                                        const uint8_t *__restrict__ dn_par, const uint32_t *__restrict__ v1,
                                                        uint32_t *__restrict__ v0, const uint64_t *__restrict__ k1,
                                                        uint64_t *__restrict__ k0, uint8_t *__restrict__ heads) {
    const uint32_t s = blockIdx.x;
    const uint64_t st = dn_start[s];
    const uint32_t len = dn_len[s];
    const bool copy = dn_par[s];
    for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < len; i += gridDim.y * 256) {  // keys: final-key sorts
        if (copy) v0[st + i] = v1[st + i];
        if (copy && k1) k0[st + i] = k1[st + i];
        heads[st + i] = i == 0;
    }
}

}  // namespace gkm
