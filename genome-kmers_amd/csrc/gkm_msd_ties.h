// gkm_msd_ties.h -- multi-word keys in the MSD sort: the groups of equal earlier key words, from
// the head flags of the order so far (bounds, run lengths, members), and their next key word.
// Private to gkm_msd.hip.  Needs no other stage header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkm_canon.h"
#include "gkm_partition.h"

namespace gkm {

// IUPAC letter -> 4-bit code: defined and uploaded (msd_tables) in gkm_msd.hip, before this header
extern __constant__ uint8_t c_code4_msd[256];

// Multi-word keys: the groups of >= 2 equal earlier words, from the head flags of the order so far.
// The first and last element of every such group, in two light passes over the head flags (no
// flag arrays): COUNT writes per 8192-element tile the numbers of group firsts and lasts; after
// their scans, STORE writes the indices from the tile's offsets (thread t owns elements
// 32 t .. 32 t + 31 of the tile, so thread order = index order).
constexpr int kTieTile = 8192;

template <bool STORE>
__global__ __launch_bounds__(256) void tie_bounds_kernel(const uint8_t *__restrict__ heads, uint64_t n,
                                                         uint32_t *__restrict__ cnt_f, uint32_t *__restrict__ cnt_l,
                                                         const uint32_t *__restrict__ off_f,
                                                         const uint32_t *__restrict__ off_l,
                                                         uint32_t *__restrict__ first, uint32_t *__restrict__ last) {
    __shared__ uint32_t s_w[2][4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTieTile + threadIdx.x * 32;
    uint32_t mf = 0, ml = 0;
    if (i0 < n) {
        // 33 head flags from i0 (past n reads as a head: the group ends there)
        uint32_t hb = 0;
        if (i0 + 33 <= n) {
            const uint4 *h4 = reinterpret_cast<const uint4 *>(heads + i0);  // i0 % 32 == 0
            const uint4 a = h4[0], b = h4[1];
            const uint32_t wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int q = 0; q < 32; ++q) hb |= (((wv[q >> 2] >> (8 * (q & 3))) & 0xFFu) != 0 ? 1u : 0u) << q;
            const bool h32 = heads[i0 + 32] != 0;
            const uint32_t nxt = (hb >> 1) | ((h32 ? 1u : 0u) << 31);  // bit q: element i0 + q + 1 is a head
            mf = hb & ~nxt;
            ml = ~hb & nxt;
        } else {
            for (int q = 0; q < 32 && i0 + q < n; ++q) {
                const bool h = heads[i0 + q] != 0, hn = i0 + q + 1 >= n || heads[i0 + q + 1] != 0;
                mf |= (h && !hn ? 1u : 0u) << q;
                ml |= (!h && hn ? 1u : 0u) << q;
            }
        }
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cf = (uint32_t)__popc(mf), cl = (uint32_t)__popc(ml);
    uint32_t inf = cf, inl = cl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t yf = __shfl_up(inf, o), yl = __shfl_up(inl, o);
        if (lane >= o) {
            inf += yf;
            inl += yl;
        }
    }
    if (lane == 63) {
        s_w[0][wave] = inf;
        s_w[1][wave] = inl;
    }
    __syncthreads();
    if (!STORE) {
        if (threadIdx.x == 0) {
            cnt_f[blockIdx.x] = s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3];
            cnt_l[blockIdx.x] = s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3];
        }
        return;
    }
    uint32_t of = off_f[blockIdx.x] + inf - cf, ol = off_l[blockIdx.x] + inl - cl;
    for (uint32_t w = 0; w < wave; ++w) {
        of += s_w[0][w];
        ol += s_w[1][w];
    }
    for (uint32_t m = mf; m; m &= m - 1) first[of++] = (uint32_t)(i0 + __ffs(m) - 1);
    for (uint32_t m = ml; m; m &= m - 1) last[ol++] = (uint32_t)(i0 + __ffs(m) - 1);
}

__global__ __launch_bounds__(256) void tie_run_lengths_kernel(const uint32_t *__restrict__ first,
                                                              uint32_t *__restrict__ last_to_len, uint64_t ng) {
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ng; g += (uint64_t)gridDim.x * 256)
        last_to_len[g] = last_to_len[g] - first[g] + 1;
}

// Key word of symbols [sym0, sym0 + nsym) of the (canonical) k-mer at p, 2-bit codes, from 17
// aligned dword loads (issued together) instead of one dependent byte load per symbol: the
// k-mer's codes as a left-aligned 128-bit value F (SWAR per dword), its reverse complement by
// two revcomp_word calls and a 128-bit shift, the smaller of the two, then the word.  k <= 64.
__device__ __forceinline__ uint32_t codes4(uint32_t w) {  // 4 bytes -> 8 bits, byte 0 on top
    uint32_t t = __builtin_bswap32(((w >> 1) ^ (w >> 2)) & 0x03030303u);
    t = (t | (t >> 6)) & 0x000F000Fu;
    return (t | (t >> 12)) & 0xFFu;
}

__device__ __forceinline__ uint64_t tie_word2(const uint8_t *sba, uint32_t p, int k, int sym0, int nsym,
                                              bool canonical) {
    // five 16-byte loads from p & ~15 (80 bytes; 17 dword loads made every k-mer 17 scattered
    // requests: C5's 113 M tie members took 19 ms)
    const uint4 *w4 = reinterpret_cast<const uint4 *>(sba + (p & ~15u));
    uint4 q[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) q[j] = w4[j];
    const uint32_t w[20] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y,
                            q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w, q[4].x, q[4].y, q[4].z, q[4].w};
    uint64_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) c0 = (c0 << 8) | codes4(w[j]);
#pragma unroll
    for (int j = 8; j < 16; ++j) c1 = (c1 << 8) | codes4(w[j]);
#pragma unroll
    for (int j = 16; j < 20; ++j) c2 = (c2 << 8) | codes4(w[j]);
    c2 <<= 32;  // symbols 64 .. 79 of the stream, on top
    // symbols 0 .. 63 from p: drop the first `off` (< 16) symbols of the stream
    const int sh = 2 * (int)(p & 15u);
    uint64_t fh = sh ? (c0 << sh) | (c1 >> (64 - sh)) : c0;
    uint64_t fl = sh ? (c1 << sh) | (c2 >> (64 - sh)) : c1;
    if (k < 64) {  // symbols past the k-mer read as 0
        if (k <= 32) {
            fh &= k == 32 ? ~0ull : ~(~0ull >> (2 * k));
            fl = 0;
        } else {
            fl &= ~(~0ull >> (2 * (k - 32)));
        }
    }
    if (canonical) {
        // reverse complement of the 64-symbol value, then shifted left past the (64 - k) pad symbols
        uint64_t rh = revcomp_word<2>(fl, 32), rl = revcomp_word<2>(fh, 32);
        const int ps = 2 * (64 - k);
        if (ps >= 64) {
            rh = rl << (ps - 64);
            rl = 0;
        } else if (ps > 0) {
            rh = (rh << ps) | (rl >> (64 - ps));
            rl <<= ps;
        }
        if (rh < fh || (rh == fh && rl < fl)) {
            fh = rh;
            fl = rl;
        }
    }
    // the word: symbols sym0 .. sym0 + nsym - 1 of (fh, fl)
    const int b0 = 2 * sym0, nb = 2 * nsym;  // bit offset from the top, width
    uint64_t x;
    if (b0 >= 64) x = fl << (b0 - 64);
    else x = b0 ? (fh << b0) | (fl >> (64 - b0)) : fh;
    return nb >= 64 ? x : x >> (64 - nb);
}

// Flat variant of tie_encode_kernel for many groups: tie_members_kernel lists every element in a group
// of >= 2 (a head flag of 0 at it or at its successor) -- 32 consecutive flags per thread from two
// 16-byte loads and one byte; COUNT per 8,192-element tile, scan, STORE at the tile's offset (one
// list append per wave on a global counter serialised 1.5 M atomics at C5: 16 ms) -- and
// tie_encode_list_kernel gives each listed element its next key word, one element per thread.  (One
// thread per element with a byte load per flag kept too few bytes in flight: 9.2 ms for C5's 3.1e9
// flags; 32 flags per thread with the members encoded in place serialised the lanes of the long
// runs of members a repeat leaves in the sorted order: 7.6 ms.)
template <bool STORE>
__global__ __launch_bounds__(256) void tie_members_kernel(const uint8_t *__restrict__ heads, uint64_t n,
                                                          uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                          uint32_t *__restrict__ list) {
    __shared__ uint32_t s_m[4][64 * 32];  // per wave: its members, in element order
    __shared__ uint32_t s_w[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kTieTile + threadIdx.x * 32;  // (as tie_bounds_kernel)
    uint32_t mem = 0;
    if (i0 + 33 <= n) {
        const uint4 *h4 = reinterpret_cast<const uint4 *>(heads + i0);  // i0 % 32 == 0
        const uint4 a = h4[0], b = h4[1];
        const uint32_t wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t hb = 0;
#pragma unroll
        for (int q = 0; q < 32; ++q) hb |= (((wv[q >> 2] >> (8 * (q & 3))) & 0xFFu) != 0 ? 1u : 0u) << q;
        const uint32_t nxt = (hb >> 1) | ((heads[i0 + 32] != 0 ? 1u : 0u) << 31);  // bit q: i0 + q + 1 is a head
        mem = ~hb | ~nxt;
    } else if (i0 < n) {
        for (int q = 0; q < 32 && i0 + q < n; ++q) {
            const uint64_t i = i0 + q;
            mem |= (heads[i] == 0 || (i + 1 < n && heads[i + 1] == 0) ? 1u : 0u) << q;
        }
    }
    const uint32_t c = (uint32_t)__popc(mem);
    const uint32_t incl = wave_incl_scan(c);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    if (!STORE) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        return;
    }
    uint32_t base = off[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) base += s_w[w];
    const uint32_t tot = s_w[wave];
    if (tot == 0) return;  // (wave-uniform)
    // the wave's members through LDS, stored by consecutive lanes (stored straight from the lanes,
    // each lane's run of up to 32 made every store instruction 64 scattered partial lines)
    uint32_t *sm = s_m[wave];
    uint32_t at = incl - c;
    for (; mem; mem &= mem - 1) sm[at++] = (uint32_t)(i0 + __ffs(mem) - 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    for (uint32_t j = lane; j < tot; j += 64) list[base + j] = sm[j];
}

template <int BITS>
__global__ __launch_bounds__(256) void tie_encode_list_kernel(const uint8_t *__restrict__ sba,
                                                              const uint32_t *__restrict__ list, uint32_t m,
                                                              const uint32_t *__restrict__ vals,
                                                              uint64_t *__restrict__ keys, int sym0, int nsym, int k,
                                                              int canonical) {
    __shared__ uint8_t s_lut4[256];
    s_lut4[threadIdx.x] = c_code4_msd[threadIdx.x];
    __syncthreads();
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const uint32_t i = list[j];
        if (BITS == 2 && k <= 64) {
            keys[i] = tie_word2(sba, vals[i], k, sym0, nsym, canonical != 0);
            continue;
        }
        const uint8_t *b = sba + vals[i];
        const bool rc = canonical && canon_is_rc<BITS>(b, k, s_lut4);
        uint64_t key = 0;
        for (int t = sym0; t < sym0 + nsym; ++t) key = (key << BITS) | canon_sym<BITS>(b, k, t, rc, s_lut4);
        keys[i] = key;
    }
}

// Multi-word keys: the next phase's key word of every element of a group of equal earlier words
// (symbols [sym0, sym0 + nsym) of its k-mer, right-aligned).  One wave per group.
template <int BITS>
__global__ __launch_bounds__(256) void tie_encode_kernel(const uint8_t *__restrict__ sba,
                                                         const uint32_t *__restrict__ g_start,
                                                         const uint32_t *__restrict__ g_len, uint32_t ngroups,
                                                         const uint32_t *__restrict__ vals, uint64_t *__restrict__ keys,
                                                         int sym0, int nsym, int k, int canonical) {
    __shared__ uint8_t s_lut4[256];
    s_lut4[threadIdx.x] = c_code4_msd[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < ngroups; g += nw) {
        const uint64_t st = g_start[g];
        const uint32_t len = g_len[g];
        if (len < 2) continue;
        for (uint32_t i = lane; i < len; i += 64) {
            if (BITS == 2 && k <= 64) {
                keys[st + i] = tie_word2(sba, vals[st + i], k, sym0, nsym, canonical != 0);
                continue;
            }
            const uint8_t *b = sba + vals[st + i];
            const bool rc = canonical && canon_is_rc<BITS>(b, k, s_lut4);
            uint64_t key = 0;
            for (int t = sym0; t < sym0 + nsym; ++t) key = (key << BITS) | canon_sym<BITS>(b, k, t, rc, s_lut4);
            keys[st + i] = key;
        }
    }
}

}  // namespace gkm
