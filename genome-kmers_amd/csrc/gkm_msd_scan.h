// gkm_msd_scan.h -- the offsets of a global level of the MSD sort: column scans of the per-tile
// digit histograms (chunk sums, bucket scan, tile apply), and the tile and chunk tables of a
// level's bucket list.
// Private to gkm_msd.hip.  Needs no other stage header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gkm_partition.h"

namespace gkm {

// ---------------------------------------------------------------------------------------------
// column-wise segmented exclusive scan of per-tile digit histograms -> per-tile digit offsets
// (one thread per digit: blockDim = RADIX)
// ---------------------------------------------------------------------------------------------
// Column scans of per-tile digit histograms.  Threads per block: min(RADIX, 1024); wider digit
// spaces (the wide L0's 2048) take blockIdx.y for the digit block (chunk sums, tile apply) or
// several consecutive digits per thread (the bucket scan).
template <int RADIX>
constexpr int scan_threads() { return RADIX < 1024 ? RADIX : 1024; }

template <int RADIX>
__global__ __launch_bounds__(scan_threads<RADIX>()) void chunk_sum_kernel(const uint32_t *__restrict__ tile_hist,
                                                          const uint32_t *__restrict__ c_first,
                                                          const uint32_t *__restrict__ c_ntiles,
                                                          uint32_t *__restrict__ chunk_hist) {
    const int d = blockIdx.y * scan_threads<RADIX>() + threadIdx.x;
    const uint64_t f = c_first[blockIdx.x];
    const uint32_t nt = c_ntiles[blockIdx.x];
    uint32_t acc = 0;
    uint32_t i = 0;
    for (; i + 8 <= nt; i += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = tile_hist[(f + i + u) * RADIX + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; i < nt; ++i) acc += tile_hist[(f + i) * RADIX + d];
    chunk_hist[(uint64_t)blockIdx.x * RADIX + d] = acc;
}

// one block per bucket: chunk bases within the bucket, digit bases, digit counts
template <int RADIX>
__global__ __launch_bounds__(scan_threads<RADIX>()) void seg_scan_kernel(uint32_t *__restrict__ chunk_hist,
                                                         const uint32_t *__restrict__ s_cfirst,
                                                         const uint32_t *__restrict__ s_nchunks,
                                                         const uint32_t *__restrict__ s_start,
                                                         uint32_t *__restrict__ seg_base, uint32_t *__restrict__ seg_cnt) {
    constexpr int TH = scan_threads<RADIX>(), DPT = RADIX / TH;  // DPT consecutive digits per thread
    __shared__ uint32_t s_wsum[TH / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t cf = s_cfirst[blockIdx.x];
    const uint32_t nc = s_nchunks[blockIdx.x];
    uint32_t run[DPT], sum = 0;
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        const int d = t * DPT + k;
        run[k] = 0;
        for (uint32_t i = 0; i < nc; ++i) {
            const uint32_t v = chunk_hist[(cf + i) * RADIX + d];
            chunk_hist[(cf + i) * RADIX + d] = run[k];
            run[k] += v;
        }
        sum += run[k];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t pre = 0;
    for (int w = 0; w < wave; ++w) pre += s_wsum[w];
    uint32_t base = s_start[blockIdx.x] + pre + incl - sum;
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        const int d = t * DPT + k;
        seg_base[(uint64_t)blockIdx.x * RADIX + d] = base;
        seg_cnt[(uint64_t)blockIdx.x * RADIX + d] = run[k];
        for (uint32_t c = 0; c < nc; ++c) chunk_hist[(cf + c) * RADIX + d] += base;
        base += run[k];
    }
}

template <int RADIX>
__global__ __launch_bounds__(scan_threads<RADIX>()) void tile_apply_kernel(uint32_t *__restrict__ tile_hist,
                                                           const uint32_t *__restrict__ c_first,
                                                           const uint32_t *__restrict__ c_ntiles,
                                                           const uint32_t *__restrict__ chunk_base) {
    const int d = blockIdx.y * scan_threads<RADIX>() + threadIdx.x;
    const uint64_t f = c_first[blockIdx.x];
    const uint32_t nt = c_ntiles[blockIdx.x];
    uint32_t run = chunk_base[(uint64_t)blockIdx.x * RADIX + d];
    uint32_t i = 0;
    for (; i + 8 <= nt; i += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = tile_hist[(f + i + u) * RADIX + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            tile_hist[(f + i + u) * RADIX + d] = run;
            run += v[u];
        }
    }
    for (; i < nt; ++i) {
        const uint32_t v = tile_hist[(f + i) * RADIX + d];
        tile_hist[(f + i) * RADIX + d] = run;
        run += v;
    }
}

// tiles, and scan chunks of ctiles tiles, of a bucket of len elements
__host__ __device__ inline uint32_t tiles_of(uint32_t len, uint32_t tile) { return (len + tile - 1) / tile; }
__host__ __device__ inline uint32_t chunks_of(uint32_t len, uint32_t tile, uint32_t ctiles) {
    return (tiles_of(len, tile) + ctiles - 1) / ctiles;
}

// tile + chunk tables of a bucket list (one thread per bucket)
// per-tile (start, count) and per-chunk (first tile, tiles) tables of the nseg buckets of a level:
// one thread per tile (j < T) and per chunk (j < C), each finding its bucket by a binary search over
// the buckets' first tile / first chunk (one thread per bucket wrote a whole bucket's tiles
// serially: 0.6 ms for the one 387 M-key bucket of a key-range rank at N = 8)
__device__ __forceinline__ uint32_t owner_of(const uint32_t *__restrict__ first, uint32_t n, uint32_t j) {
    uint32_t lo = 0, hi = n;  // the last bucket with first <= j
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void tile_table_kernel(const uint32_t *__restrict__ s_start,
                                                         const uint32_t *__restrict__ s_len,
                                                         const uint32_t *__restrict__ s_tfirst,
                                                         const uint32_t *__restrict__ s_cfirst, uint32_t nseg,
                                                         uint32_t tile, uint32_t T, uint32_t C, uint32_t ctiles,
                                                         uint32_t *__restrict__ t_start,
                                                         uint32_t *__restrict__ t_count, uint32_t *__restrict__ c_first,
                                                         uint32_t *__restrict__ c_ntiles) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < T) {
        const uint32_t s = owner_of(s_tfirst, nseg, j);
        const uint32_t r = j - s_tfirst[s], len = s_len[s];
        t_start[j] = s_start[s] + r * tile;
        t_count[j] = std::min<uint32_t>(tile, len - r * tile);
    }
    if (j < C) {
        const uint32_t s = owner_of(s_cfirst, nseg, j);
        const uint32_t r = j - s_cfirst[s], nt = (s_len[s] + tile - 1) / tile;
        c_first[j] = s_tfirst[s] + r * ctiles;
        c_ntiles[j] = std::min<uint32_t>(ctiles, nt - r * ctiles);
    }
}

__global__ __launch_bounds__(256) void seg_counts_kernel(const uint32_t *__restrict__ s_len, uint32_t nseg,
                                                         uint32_t tile, uint32_t ctiles, uint32_t *__restrict__ ntiles,
                                                         uint32_t *__restrict__ nchunks) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const uint32_t nt = (s_len[s] + tile - 1) / tile;
    ntiles[s] = nt;
    nchunks[s] = (nt + ctiles - 1) / ctiles;
}

// seg_counts_kernel and the exclusive scans of both counts in ONE workgroup, for the level's
// bucket list of up to kSegScanMax entries (C3: 128 / 32 K buckets; the deep levels of a repeat-rich
// genome: tens): one launch instead of seven, the totals already known from the list counters
constexpr uint32_t kSegScanMax = 1u << 16;
__global__ __launch_bounds__(1024) void seg_tiles_scan_kernel(const uint32_t *__restrict__ s_len, uint32_t nseg,
                                                              uint32_t tile, uint32_t ctiles,
                                                              uint32_t *__restrict__ tfirst,
                                                              uint32_t *__restrict__ cfirst,
                                                              uint32_t *__restrict__ nchunks) {
    __shared__ uint32_t s_w[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry_t = 0, carry_c = 0;
    for (uint32_t b0 = 0; b0 < nseg; b0 += 1024) {  // (block-uniform)
        const uint32_t s = b0 + tid;
        const uint32_t nt = s < nseg ? tiles_of(s_len[s], tile) : 0, nc = (nt + ctiles - 1) / ctiles;
        const uint32_t it = wave_incl_scan(nt), ic = wave_incl_scan(nc);
        if (lane == 63) {
            s_w[0][wave] = it;
            s_w[1][wave] = ic;
        }
        __syncthreads();
        uint32_t pt = carry_t, pc = carry_c;
        for (int w = 0; w < 16; ++w) {
            const uint32_t a = s_w[0][w], d = s_w[1][w];
            if (w < wave) {
                pt += a;
                pc += d;
            }
            carry_t += a;
            carry_c += d;
        }
        if (s < nseg) {
            tfirst[s] = pt + it - nt;
            cfirst[s] = pc + ic - nc;
            nchunks[s] = nc;
        }
        __syncthreads();
    }
}

}  // namespace gkm
