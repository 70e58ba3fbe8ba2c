// gkm_msd_l0.h -- L0 of the MSD sort: keys straight from the sequence byte array.  The count and
// partition kernels over packed tiles, the key-range shards' select and ownership kernels, the
// 2-bit packed copy of the sequence, and the keys of received starts from that copy.
// Private to gkm_msd.hip.  Needs gkm_msd_config.h and no other stage header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkm_canon.h"
#include "gkm_internal.h"
#include "gkm_msd_config.h"
#include "gkm_partition.h"
#include "gkm_swar.h"

namespace gkm {

// IUPAC letter -> 4-bit code: defined and uploaded (msd_tables) in gkm_msd.hip, before this header
extern __constant__ uint8_t c_code4_msd[256];

// ---------------------------------------------------------------------------------------------
// L0: keys straight from the sequence byte array
// ---------------------------------------------------------------------------------------------
// A tile's bases are first packed into LDS: symbol codes MSB-first (64/BITS per word) and a '$'
// bitmask (32 positions per word).  The key of position p is then one funnel shift of two code
// words, and p is a valid start iff the S mask bits from p are all zero ('$' ends a contig; the
// pad after the array is '$').
struct L0Args {
    const uint8_t *sba;
    uint64_t lo, hi;  // k-mer starts in [lo, hi) (lo a multiple of 32: 16-B aligned tiles)
    int symbols, total_bits;
    int acgt_only;    // 2-bit keys of a mixed sba: k-mers holding a non-ACGT byte are not started
    // key-range shard: only k-mers whose ownership digit o (the top own_bits key bits) has
    // o - own_lo < own_span are kept (all: 0, ~0)
    uint32_t own_lo = 0, own_span = 0xFFFFFFFFu;
    int own_bits = 7;
    // 2-bit packed copy of an ACGT sba (pack2_kernel, 32 positions per word; null: pack bytes)
    const uint64_t *pk_code = nullptr;
    const uint32_t *pk_dol = nullptr;
    // unused: holds the place of a removed profiling pointer.  Every L0 kernel takes this struct by
    // value, and dropping the 8 bytes moves the kernel arguments behind it, which changed the
    // register allocation of the tuned kernels (other SGPR spill counts in msd0_pipe_kernel); to be
    // removed together with an A/B run of the L0 passes
    uint64_t reserved = 0;
};

__device__ __forceinline__ bool l0_owned(uint32_t d, const L0Args &a) { return d - a.own_lo < a.own_span; }
// the ownership digit of a total_bits-bit key (own_bits <= total_bits)
__device__ __forceinline__ bool l0_owned_key(uint64_t key, const L0Args &a) {
    return l0_owned((uint32_t)(key >> (a.total_bits - a.own_bits)), a);
}

template <int BITS, int TILE>
struct L0Pack {
    static constexpr int kGroups = TILE / 32 + 3;             // 32-position groups packed (k <= 64)
    static constexpr int kCodeWords = kGroups * BITS / 2 + 1;  // u64 words (+1 for the funnel)
};

// The tile's bytes (kGroups * 32, incl. the halo) in 8-byte units, spread over all T threads:
// thread t holds units t, t + T, ... (kPer registers; index clamped so the loads stay branch-free)
template <int BITS, int TILE, int T>
struct L0Units {
    static constexpr int kUnits = L0Pack<BITS, TILE>::kGroups * 4;
    static constexpr int kPer = (kUnits + T - 1) / T;
};

template <int BITS, int TILE, int T>
__device__ __forceinline__ void l0_load(const L0Args &a, uint64_t P0, uint64_t (&r)[L0Units<BITS, TILE, T>::kPer]) {
    using U = L0Units<BITS, TILE, T>;
    static_assert(U::kPer >= 2, "the packed path keeps a code word and a stop word");
    // every element of r is written on both paths (a path that leaves some unwritten made the
    // compiler keep r in scratch memory at kPer = 3)
    if (BITS == 2 && a.pk_code) {  // pre-packed: thread t holds the words of groups t, t + T, ...
        constexpr int kPairs = U::kPer / 2;
        static_assert(kPairs * T >= L0Pack<BITS, TILE>::kGroups, "every packed group has a register pair");
#pragma unroll
        for (int j = 0; j < kPairs; ++j) {
            const uint64_t g = (P0 >> 5) + min((uint32_t)(threadIdx.x + j * T), (uint32_t)L0Pack<BITS, TILE>::kGroups - 1);
            r[2 * j] = a.pk_code[g];
            r[2 * j + 1] = a.pk_dol[g];
        }
#pragma unroll
        for (int j = 2 * kPairs; j < U::kPer; ++j) r[j] = 0;
    } else {
        const uint64_t *s8 = reinterpret_cast<const uint64_t *>(a.sba + P0);
#pragma unroll
        for (int j = 0; j < U::kPer; ++j) r[j] = s8[min((uint32_t)(threadIdx.x + j * T), (uint32_t)U::kUnits - 1)];
    }
}

// 2-bit codes (A0 C1 G2 T3) of 8 bytes as 16 bits, position 0 in the most significant pair
__device__ __forceinline__ uint32_t pack2_8(uint64_t x) {
    uint64_t t = __builtin_bswap64(((x >> 1) ^ (x >> 2)) & 0x0303030303030303ull);
    t = (t | (t >> 6)) & 0x000F000F000F000Full;
    t = (t | (t >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((t | (t >> 24)) & 0xFFFFu);
}

// s_dol bit = the position ends k-mers: '$' (or, acgt_only, any byte outside ACGT).  Every thread
// packs its 8-byte units: 2-bit codes into 16-bit (4-bit: 32-bit) pieces of the MSB-first code
// words, stop flags into bytes of the 32-position mask words.
template <int BITS, int TILE, int T>
__device__ __forceinline__ void l0_pack(const uint64_t (&r)[L0Units<BITS, TILE, T>::kPer], uint64_t *s_code,
                                        uint32_t *s_dol, const uint8_t *lut4, int acgt_only, bool packed) {
    using U = L0Units<BITS, TILE, T>;
    using P = L0Pack<BITS, TILE>;
    constexpr uint64_t kOnes = 0x0101010101010101ull;
    if (BITS == 2 && packed) {
#pragma unroll
        for (int j = 0; j < U::kPer / 2; ++j) {
            const uint32_t g = threadIdx.x + j * T;
            if (g < (uint32_t)P::kGroups) {
                s_code[g] = r[2 * j];
                s_dol[g] = (uint32_t)r[2 * j + 1];
            }
        }
        if (threadIdx.x == 0) s_code[P::kCodeWords - 1] = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < U::kPer; ++j) {
        const uint32_t u = threadIdx.x + j * T;
        if (u < (uint32_t)U::kUnits) {
            const uint64_t x = r[j];
            uint64_t z;
            if (acgt_only)
                z = non_acgt_bytes(x);
            else
                z = zero_bytes(x ^ (kOnes * GK_DOLLAR));
            reinterpret_cast<uint8_t *>(s_dol)[(u & ~3u) + 3 - (u & 3u)] = (uint8_t)gather_flags8(z);
            if (BITS == 2) {
                reinterpret_cast<uint16_t *>(s_code)[(u & ~3u) + 3 - (u & 3u)] = (uint16_t)pack2_8(x);
            } else {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 8; ++b) v = (v << 4) | lut4[(x >> (8 * b)) & 0xFFu];
                reinterpret_cast<uint32_t *>(s_code)[(u & ~1u) + 1 - (u & 1u)] = v;
            }
        }
    }
    if (threadIdx.x == 0) s_code[P::kCodeWords - 1] = 0;
}

template <int BITS>
__device__ __forceinline__ uint64_t l0_key(const uint64_t *s_code, uint32_t p, int B) {
    const uint32_t o = p * BITS, w = o >> 6, s = o & 63;
    uint64_t x = s_code[w] << s;
    if (s) x |= s_code[w + 1] >> (64 - s);
    return x >> (64 - B);
}

// CANON: the first key word of the canonical k-mer (gkm_canon.h) is the smaller of the first word
// of the k-mer and the first word of its reverse complement -- the reverse complement of the
// k-mer's last B / BITS symbols.  (If the two are equal the whole-k-mer choice does not change the
// first word; later words are decided in tie_encode_kernel.)
template <int BITS, bool CANON>
__device__ __forceinline__ uint64_t l0_key_of(const uint64_t *s_code, uint32_t p, int B, int k) {
    const uint64_t f = l0_key<BITS>(s_code, p, B);
    if (!CANON) return f;
    const int n = B / BITS;
    const uint64_t r = revcomp_word<BITS>(l0_key<BITS>(s_code, p + k - n, B), n);
    return r < f ? r : f;
}

__device__ __forceinline__ bool l0_valid(const uint32_t *s_dol, uint32_t p, int S) {
    const uint32_t w = p >> 5, s = p & 31;
    const uint64_t x = (((uint64_t)s_dol[w] << 32) | s_dol[w + 1]) << s;
    if (S <= 32) return (x >> (64 - S)) == 0;
    // multi-word keys (33 <= S <= 64): the first 32 positions, then the rest from p + 32
    const uint64_t y = (((uint64_t)s_dol[w + 1] << 32) | s_dol[w + 2]) << s;
    return (x >> 32) == 0 && (y >> (96 - S)) == 0;
}

// Eight consecutive positions q0 .. q0 + 7 (q0 % 8 == 0) of a packed 2-bit tile from one 128-bit
// code window and one 64-position stop window: keep mask (valid, before a.hi, owned) and the keys
// (only if `keys`) or the L0 digits.  When no lane of the wave sees a stop or the sequence end and
// the L0 digit is the top 7 bits of a key of >= 8 bits, the digits come straight from the window's
// high half (bits [25 - 2i, 32 - 2i)) -- a shift, a mask and a compare per position.
struct Win8 {
    uint64_t T, T2;  // symbols q0 .., q0 + 32 ..
    uint64_t D;      // stops q0 .. q0 + 63, MSB first
};

__device__ __forceinline__ Win8 win8_load(const uint64_t *s_code, const uint32_t *s_dol, uint32_t q0) {
    const uint32_t w0 = q0 >> 5, s0 = (q0 & 31) * 2;  // s0 in {0, 16, 32, 48}
    const uint64_t A0 = s_code[w0], A1 = s_code[w0 + 1], A2 = s_code[w0 + 2];
    Win8 w;
    w.T = s0 ? (A0 << s0) | (A1 >> (64 - s0)) : A0;
    w.T2 = s0 ? (A1 << s0) | (A2 >> (64 - s0)) : A1;
    const uint32_t ds = q0 & 31;  // in {0, 8, 16, 24}
    const uint64_t D0 = ((uint64_t)s_dol[w0] << 32) | s_dol[w0 + 1];
    w.D = ds ? (D0 << ds) | (s_dol[w0 + 2] >> (32 - ds)) : D0;
    return w;
}

__device__ __forceinline__ uint64_t win8_key(const Win8 &w, int i, int B) {
    const uint64_t Ti = i ? (w.T << (2 * i)) | (w.T2 >> (64 - 2 * i)) : w.T;
    return B >= 64 ? Ti : Ti >> (64 - B);
}

// the 32 symbols from position q of a packed 2-bit tile, MSB first (any q)
__device__ __forceinline__ uint64_t win32_at(const uint64_t *s_code, uint32_t q) {
    const uint32_t w = q >> 5, s = (q & 31) * 2;
    return s ? (s_code[w] << s) | (s_code[w + 1] >> (64 - s)) : s_code[w];
}

// wave-uniform call (a ballot inside)
__device__ __forceinline__ uint32_t win8_keep(const Win8 &w, const L0Args &a, Dig d0, int64_t left,
                                              const uint32_t *s_dol, uint32_t q0, uint32_t (&dig)[8]) {
    const uint32_t Th = (uint32_t)(w.T >> 32);
    const bool top7 = d0.mask == 0x7Fu && (int)d0.shift == a.total_bits - 7 && a.symbols <= 56;
    uint32_t keepm = 0;
    // ownership digits of up to 18 bits come from the same 32-bit window (2 i + own_bits <= 32)
    const uint32_t omask = (1u << a.own_bits) - 1;
    if (top7 && a.own_bits <= a.total_bits && a.own_bits <= 18 && __ballot(w.D != 0 || left < 8) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dig[i] = (Th >> (25 - 2 * i)) & 0x7Fu;
            keepm |= (l0_owned((Th >> (32 - 2 * i - a.own_bits)) & omask, a) ? 1u : 0u) << i;
        }
        return keepm;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t key = win8_key(w, i, a.total_bits);
        dig[i] = dg_of(key, d0);
        const uint64_t Di = w.D << i;
        const bool valid = a.symbols <= 56 ? (Di == 0 || (int)__clzll((long long)Di) >= a.symbols)
                                           : l0_valid(s_dol, q0 + i, a.symbols);
        keepm |= ((valid && i < left && l0_owned_key(key, a)) ? 1u : 0u) << i;
    }
    return keepm;
}

template <int BITS, int T, int I, int R, bool CANON = false>
__global__ __launch_bounds__(T) void msd0_count_kernel(L0Args a, Dig d0, uint32_t *__restrict__ tile_hist,
                                                       uint32_t ntiles) {
    constexpr int TILE = T * I;
    constexpr int RADIX = 1 << R;
    using P = L0Pack<BITS, TILE>;
    __shared__ uint64_t s_code[P::kCodeWords];
    __shared__ uint32_t s_dol[P::kGroups];
    // 4 interleaved histogram copies (digit d, copy c at 4 d + c; copy = thread & 3): the lanes of
    // one atomic that share a digit land on 4 different words in 4 banks (C3: 1.845 -> 1.797 ms, A/B)
    constexpr int NC = 4;
    __shared__ uint32_t s_hist[RADIX * NC];
    __shared__ uint8_t s_lut4[256];
    const int t = threadIdx.x;
    if (t < 256) s_lut4[t] = c_code4_msd[t];
    // persistent: the next tile's bytes are loaded while this one is counted
    uint64_t rr[L0Units<BITS, TILE, T>::kPer];
    if (blockIdx.x < ntiles) l0_load<BITS, TILE, T>(a, a.lo + (uint64_t)blockIdx.x * TILE, rr);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t P0 = a.lo + (uint64_t)tile * TILE;
        // each thread zeroes the copies it summed for the previous tile (no barrier between)
        for (int i = t; i < RADIX; i += T)
#pragma unroll
            for (int c = 0; c < NC; ++c) s_hist[i * NC + c] = 0;
        lds_barrier();  // the LUT; the previous tile's histogram and codes have been read
        l0_pack<BITS, TILE, T>(rr, s_code, s_dol, s_lut4, a.acgt_only, a.pk_code != nullptr);
        lds_barrier();
        if (tile + gridDim.x < ntiles) l0_load<BITS, TILE, T>(a, P0 + (uint64_t)gridDim.x * TILE, rr);
        if constexpr (BITS == 2 && !CANON) {  // 8 consecutive positions per thread (Win8)
            static_assert(TILE % 8 == 0 && (TILE / 8) % 64 == 0, "whole waves per round");
            for (uint32_t g = t; g < TILE / 8; g += T) {
                const uint32_t q0 = g * 8;
                const Win8 w = win8_load(s_code, s_dol, q0);
                uint32_t dig[8];
                const uint32_t keepm = win8_keep(w, a, d0, (int64_t)a.hi - (int64_t)(P0 + q0), s_dol, q0, dig);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if ((keepm >> i) & 1u) atomicAdd(&s_hist[dig[i] * NC + (t & (NC - 1))], 1u);
            }
        } else {
            // canonical 2-bit keys in a tile without stops: the digit is the smaller of the forward
            // and the reverse-complement top 7 bits, 8 consecutive positions per thread from two
            // 32-symbol windows (at q0 and at q0 + k - 4)
            bool fast = false;
            if constexpr (BITS == 2 && CANON && (R == 7 || R == 8)) {
                uint32_t anystop = 0;
                for (int j = t; j < P::kGroups; j += T) anystop |= s_dol[j];
                // (ownership digits other than the L0 digit -- the key-range ranks' 12 bits -- take the
                // per-position path below)
                fast = __syncthreads_or(anystop != 0) == 0 && P0 + TILE <= a.hi &&
                       (d0.mask == 0x7Fu || d0.mask == 0xFFu) && (int)d0.shift == a.total_bits - R &&
                       a.symbols >= 4 && (a.own_span == 0xFFFFFFFFu || a.own_bits == R);
                if (fast) {
                    for (uint32_t g = t; g < TILE / 8; g += T) {
                        const uint32_t q0 = g * 8;
                        // only the top 32 bits of each window are read (16 symbols: positions q0 .. q0 + 10,
                        // q0 + k - 4 .. q0 + k + 6): 32-bit shifts per position instead of 64-bit ones
                        // (the 64-bit form ran this pass VALU-bound at 5.0 ms for C5)
                        const uint32_t tf = (uint32_t)(win32_at(s_code, q0) >> 32);
                        const uint32_t tr = (uint32_t)(win32_at(s_code, q0 + a.symbols - 4) >> 32);
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            // (R = 8: the top 8 bits of both words; the smaller digit is the top of the smaller word)
                            const uint32_t f7 = (tf >> (32 - R - 2 * i)) & ((1u << R) - 1);
                            const uint32_t v = (tr >> (24 - 2 * i)) & 0xFFu;  // symbols q0+k-4+i ..
                            const uint32_t rv = ((v & 3u) << 6) | ((v & 0xCu) << 2) | ((v >> 2) & 0xCu) | (v >> 6);
                            const uint32_t d = min(f7, (~rv & 0xFFu) >> (8 - R));
                            if (l0_owned(d, a)) atomicAdd(&s_hist[d * NC], 1u);
                        }
                    }
                }
            }
            if (!fast) {
                // (tiles with stops, or the sequence end).  Canonical keys: two windows and a
                // reverse complement per position -- a loop, not unrolled, so the fast path above
                // keeps its registers (unrolled over the 96 positions it took 256 VGPRs, spilled
                // to scratch and ran the whole kernel at one wave per SIMD).  4-bit forward keys
                // (every tile takes this path): unrolled by 4 (fully unrolled: 256 VGPRs + 206
                // AGPRs, one wave per SIMD)
                constexpr int UNR = CANON ? 1 : 4;
#pragma unroll UNR
                for (int i = 0; i < I; ++i) {
                    const uint32_t p = i * T + t;
                    const uint64_t key = l0_key_of<BITS, CANON>(s_code, p, a.total_bits, a.symbols);
                    const uint32_t d = dg_of(key, d0);
                    if (l0_valid(s_dol, p, a.symbols) && P0 + p < a.hi && l0_owned_key(key, a))
                        atomicAdd(&s_hist[d * NC], 1u);
                }
            }
        }
        lds_barrier();
        for (int i = t; i < RADIX; i += T) {
            uint32_t h = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) h += s_hist[i * NC + c];
            tile_hist[(uint64_t)tile * RADIX + i] = h;
        }
    }
}

// L0 partition, software-pipelined with position staging.  The L0 input is the packed tile
// itself, so a staged element needs only its tile position (u16): its key is re-derived from the
// tile's codes when it is stored, and its start is the tile base + position.  Positions and codes
// are double-buffered (2 x (48 + 6) KB at 24,576 positions), so the previous tile's stores are
// spread over EVERY phase of this tile -- packing, ranking, scan, staging -- and the memory pipe
// never idles (staged as (key, start) in one 135 KB buffer, the stores had to finish before the
// staging: a phase profile showed them issued in 45 % of the tile time, backed up, and the pipe
// idle for the rest).  Twice the tile of the level passes: runs of ~192 per digit.
#ifndef GKM_L0_T
#define GKM_L0_T 1024
#endif
#ifndef GKM_L0_I
#define GKM_L0_I 24
#endif
// (tuning overrides, tools/build_variant.sh: GKM_L0_T threads x GKM_L0_I positions per tile)
constexpr int kP0T = GKM_L0_T;           // L0 tile: kP0T threads x kP0I positions
constexpr int kP0I = GKM_L0_I;
constexpr int kP0Tile = kP0T * kP0I;     // 24,576 (< 65,536: positions staged as u16)

// P88 (the packed L0, round 5): each element leaves as the level-1 digit byte (nd), the key bits below
// it above the start's high bits (u64: key << shi | start >> (32 - shi)) and the start's low bits
// (u16 in nd.out16) -- 11 B instead of 13 (key, start, digit); the level behind reads it (INP = 2)
// OWN (the key-range ranks' fused select, round 5): only k-mers whose ownership digit (the top
// a.own_bits key bits) is in the rank's range are partitioned -- the select pass and its 13-byte
// round trip per kept k-mer fall away
template <int BITS, int T, int I, int R, bool ND, bool CANON = false, bool P88 = false, bool OWN = false>
__global__ __launch_bounds__(T) void msd0_pipe_kernel(L0Args a, Dig d0, const uint32_t *__restrict__ tile_off,
                                                      uint64_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                      uint32_t ntiles, uint64_t sink, NextDigits nd) {
    constexpr int TILE = T * I;
    static_assert(TILE < 65536, "tile positions are staged as u16");
    constexpr int RADIX = 1 << R;
    constexpr int NW = T / 64;
    // store groups of the previous tile: G_TOP after the packing, one per ranked item, G_SCAN
    // during the scan, the rest after the staging
#ifndef GKM_L0_GTOP
#define GKM_L0_GTOP 1
#endif
#ifndef GKM_L0_GSCAN
#define GKM_L0_GSCAN 2
#endif
    // (tuning overrides, tools/gpu_ab_l0_groups.sh: G_TOP 1 beat 0, 2 and 4 by 0.2-0.6 ms at C3)
    constexpr int G_TOP = GKM_L0_GTOP, G_SCAN = GKM_L0_GSCAN;
    constexpr int G_RANK = I - G_TOP - G_SCAN - 2 > 0 ? I - G_TOP - G_SCAN - 2 : 0;
    using P = L0Pack<BITS, TILE>;
    static_assert(T >= RADIX, "one thread per digit");
    __shared__ uint16_t s_pos[2][TILE + 2];          // positions in digit order (slot TILE: sink)
    __shared__ uint64_t s_code[2][P::kCodeWords];   // this tile's and the staged tile's codes
    __shared__ uint32_t s_dol[P::kGroups];
    __shared__ uint32_t s_wc[NW * RADIX];
    __shared__ uint32_t s_toff[2][RADIX];
    __shared__ uint32_t s_start[RADIX + 1];
    __shared__ uint32_t s_wsum[RADIX / 64 > 0 ? RADIX / 64 : 1];
    __shared__ uint8_t s_lut4[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) s_lut4[tid] = c_code4_msd[tid];
    // the first iteration's stores read buffer 1 before anything was staged (they go to the
    // sink): keep their positions inside the tile
    for (int i = tid; i < TILE + 2; i += T) s_pos[1][i] = 0;
    lds_barrier();  // the LUT, read by every thread's pack
    const TileWalk walk(ntiles);
    uint64_t rr[L0Units<BITS, TILE, T>::kPer];
    uint32_t toff = 0;
    auto load = [&](uint32_t t) {
        toff = tile_off[(uint64_t)t * RADIX + (tid & (RADIX - 1))];
        l0_load<BITS, TILE, T>(a, a.lo + (uint64_t)t * TILE, rr);
    };
    uint32_t pcnt = 0;  // staged elements of the previous tile (0: none -> its stores go to the sink)
    uint64_t pP0 = 0;   // the previous tile's first position
    int b = 0;          // this tile's buffers; b ^ 1: the staged previous tile
    // one store group of the previous tile: slot s -> position -> key (from the staged codes)
    auto store_group = [&](int g) {
        const uint32_t s = min((uint32_t)(tid + g * T), pcnt - 1);  // pcnt == 0: stays in the tile
        const uint32_t p = s_pos[b ^ 1][s];
        const uint64_t key = l0_key_of<BITS, CANON>(s_code[b ^ 1], p, a.total_bits, a.symbols);
        const uint64_t o = pcnt ? (uint64_t)(s_toff[b ^ 1][dg_of(key, d0)] + s) : sink;
        if (P88) {
            const uint32_t st = (uint32_t)(pP0 + p);
            const int shi = nd.pshi;
            kout[o] = (key << shi) | (st >> (32 - shi));  // (the sorted and digit bits shift out)
            nd.out16[o] = (uint16_t)(st & ((1u << (32 - shi)) - 1));
            nd.out[o] = (uint8_t)dg_of(key, nd.d);
        } else {
            if (kout) kout[o] = key;  // (none: a starts-only shard send, GK_SHARD_STARTS_ONLY)
            vout[o] = (uint32_t)(pP0 + p);
            if (ND) nd.out[o] = (uint8_t)dg_of(key, nd.d);
        }
        // keep each group's loads and stores in place: hoisting the groups' LDS reads ahead (the
        // scheduler's choice) keeps 22 groups' positions and keys live and spills them to scratch,
        // whose vmcnt waits then drain every store in flight
        __builtin_amdgcn_sched_barrier(0);
    };
    if (walk.first < walk.end) load(walk.first);
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    for (uint32_t t = walk.first; t < walk.end; t += walk.step) {
        uint32_t *wc = s_wc + wave * RADIX;
#pragma unroll
        for (int u = 0; u < (RADIX + 63) / 64; ++u)
            if (u * 64 + lane < RADIX) wc[u * 64 + lane] = 0;
        if (tid < RADIX) s_toff[b][tid] = toff;
        l0_pack<BITS, TILE, T>(rr, s_code[b], s_dol, s_lut4, a.acgt_only, a.pk_code != nullptr);
        // rr and toff are consumed: the next tile's bytes fly during this whole tile (the last
        // tile re-loads itself, so every iteration issues the same loads: static wait counts)
        load(min(t + walk.step, walk.end - 1));
#pragma unroll
        for (int g = 0; g < G_TOP; ++g) store_group(g);
        lds_barrier();  // packed codes visible
        const uint64_t P0 = a.lo + (uint64_t)t * TILE;
        // a tile without stops that ends before a.hi: every position starts a k-mer (wave-uniform)
        uint32_t anystop = 0;
#pragma unroll
        for (int j = 0; j < (P::kGroups + 63) / 64; ++j)
            anystop |= s_dol[min((uint32_t)(j * 64 + lane), (uint32_t)P::kGroups - 1)];
        const bool clean = __ballot(anystop != 0) == 0 && P0 + TILE <= a.hi;
        uint32_t dr[I], validm = 0;  // per item: digit | rank << 8 (rank < I * 64)
        uint32_t p0 = wave * (I * 64) + lane;
        asm volatile("" : "+v"(p0));
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const uint32_t p = p0 + i * 64;
            const uint64_t key = l0_key_of<BITS, CANON>(s_code[b], p, a.total_bits, a.symbols);
            bool valid = clean || (l0_valid(s_dol, p, a.symbols) && P0 + p < a.hi);
            if (OWN) valid = valid && l0_owned_key(key, a);
            validm |= (valid ? 1u : 0u) << i;
            const uint32_t dig = dg_of(key, d0);
            // stable rank by one returning LDS atomic (rank_atomic, gkm_partition.h); the LDS-mask
            // round trip it replaces took C3 L0 14.0 -> 12.9 ms against R + 1 ballots per item
            dr[i] = dig | (rank_atomic(wc, dig, valid) << 8);
            if (i < G_RANK) store_group(G_TOP + i);
            __builtin_amdgcn_sched_barrier(0);  // one item at a time (register pressure, see above)
        }
        lds_barrier();  // ranks final
        uint32_t total = 0, incl = 0;
        if (tid < RADIX) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t v = s_wc[w * RADIX + tid];
                s_wc[w * RADIX + tid] = total;
                total += v;
            }
            incl = wave_incl_scan(total);
            if (lane == 63) s_wsum[wave] = incl;
        }
#pragma unroll
        for (int g = 0; g < G_SCAN; ++g) store_group(G_TOP + G_RANK + g);
        lds_barrier();
        if (tid < RADIX) {
            uint32_t pre = 0;
            for (int w = 0; w < wave; ++w) pre += s_wsum[w];
            const uint32_t st = pre + incl - total;
            s_start[tid] = st;
            s_toff[b][tid] -= st;
            if (tid == RADIX - 1) s_start[RADIX] = pre + incl;
        }
        lds_barrier();
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const bool valid = (validm >> i) & 1u;
            const uint32_t dg = dr[i] & 0xFFu;
            const uint32_t sl = valid ? s_start[dg] + wc[dg] + (dr[i] >> 8) : (uint32_t)TILE;
            s_pos[b][sl] = (uint16_t)(p0 + i * 64);
        }
        const uint32_t cnt = s_start[RADIX];
#pragma unroll
        for (int g = G_TOP + G_RANK + G_SCAN; g < I; ++g) store_group(g);
        pcnt = cnt;
        pP0 = P0;
        lds_barrier();  // staging complete; counters, codes and the previous staging read
        b ^= 1;
    }
    if (walk.first < walk.end) {
#pragma unroll
        for (int g = 0; g < I; ++g) store_group(g);
    }
}

// Wide L0 partition (R = 10 or 11 bits; 2-bit keys of one word, forward): the
// position-staged, software-pipelined scheme of msd0_pipe_kernel with a digit space the 7-bit one
// cannot hold -- per-wave u16 counters, two per word (rank_atomic16), K = RADIX / T digits per
// thread in the scan, K tile offsets per thread.  With the level pass behind it, 11 + 8 bits leave
// the C3 buckets at ~5.9 K keys, finished in one block-local round (three passes instead of
// four global ones plus the wave-local round).
template <int T, int I, int R, bool ND>
__global__ __launch_bounds__(T) void msd0_wide_kernel(L0Args a, Dig d0, const uint32_t *__restrict__ tile_off,
                                                      uint64_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                      uint32_t ntiles, uint64_t sink, NextDigits nd) {
    constexpr int TILE = T * I;
    static_assert(TILE < 65536, "tile positions are staged as u16");
    constexpr int RADIX = 1 << R;
    constexpr int NW = T / 64;
    constexpr int K = RADIX / T;  // digits per thread in the scan
    static_assert(RADIX % T == 0 && K >= 1, "whole digits per thread");
    static_assert(I * 64 < 65536, "per-wave counts fit 16 bits");
    constexpr int G_TOP = 1, G_SCAN = 2;
    constexpr int G_RANK = I - G_TOP - G_SCAN - 2 > 0 ? I - G_TOP - G_SCAN - 2 : 0;
    using P = L0Pack<2, TILE>;
    __shared__ uint16_t s_pos[2][TILE + 2];          // positions in digit order (slot TILE: sink)
    __shared__ uint64_t s_code[2][P::kCodeWords];   // this tile's and the staged tile's codes
    __shared__ uint32_t s_dol[P::kGroups];
    __shared__ uint32_t s_wc[NW * RADIX / 2];        // per-wave u16 digit counters
    __shared__ uint32_t s_toff[2][RADIX];
    __shared__ uint32_t s_start[RADIX + 1];
    __shared__ uint32_t s_wsum[NW];
    uint16_t *const s_wc16 = reinterpret_cast<uint16_t *>(s_wc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < TILE + 2; i += T) s_pos[1][i] = 0;
    lds_barrier();
    const TileWalk walk(ntiles);
    uint64_t rr[L0Units<2, TILE, T>::kPer];
    uint32_t toff[K];
    auto load = [&](uint32_t t) {
#pragma unroll
        for (int k = 0; k < K; ++k) toff[k] = tile_off[(uint64_t)t * RADIX + tid * K + k];
        l0_load<2, TILE, T>(a, a.lo + (uint64_t)t * TILE, rr);
    };
    uint32_t pcnt = 0;
    uint64_t pP0 = 0;
    int b = 0;
    auto store_group = [&](int g) {
        const uint32_t s = min((uint32_t)(tid + g * T), pcnt - 1);
        const uint32_t p = s_pos[b ^ 1][s];
        const uint64_t key = l0_key<2>(s_code[b ^ 1], p, a.total_bits);
        const uint64_t o = pcnt ? (uint64_t)(s_toff[b ^ 1][dg_of(key, d0)] + s) : sink;
        kout[o] = key;
        vout[o] = (uint32_t)(pP0 + p);
        if (ND) nd.out[o] = (uint8_t)dg_of(key, nd.d);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (walk.first < walk.end) load(walk.first);
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    for (uint32_t t = walk.first; t < walk.end; t += walk.step) {
        uint32_t *wc = s_wc + wave * (RADIX / 2);
#pragma unroll
        for (int u = 0; u < RADIX / 2 / 64; ++u) wc[u * 64 + lane] = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) s_toff[b][tid * K + k] = toff[k];
        l0_pack<2, TILE, T>(rr, s_code[b], s_dol, nullptr, 0, a.pk_code != nullptr);
        load(min(t + walk.step, walk.end - 1));
#pragma unroll
        for (int g = 0; g < G_TOP; ++g) store_group(g);
        lds_barrier();  // packed codes visible
        const uint64_t P0 = a.lo + (uint64_t)t * TILE;
        uint32_t anystop = 0;
#pragma unroll
        for (int j = 0; j < (P::kGroups + 63) / 64; ++j)
            anystop |= s_dol[min((uint32_t)(j * 64 + lane), (uint32_t)P::kGroups - 1)];
        const bool clean = __ballot(anystop != 0) == 0 && P0 + TILE <= a.hi;
        uint32_t dr[I];  // per item: digit | rank << R, all ones when not valid
        uint32_t p0 = wave * (I * 64) + lane;
        asm volatile("" : "+v"(p0));
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const uint32_t p = p0 + i * 64;
            const bool valid = clean || (l0_valid(s_dol, p, a.symbols) && P0 + p < a.hi);
            const uint32_t dig = dg_of(l0_key<2>(s_code[b], p, a.total_bits), d0);
            const uint32_t rk = rank_atomic16<R>(wc, dig, valid);
            dr[i] = valid ? dig | (rk << R) : ~0u;
            if (i < G_RANK) store_group(G_TOP + i);
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_barrier();  // ranks final
        // per-digit totals over the waves -> per-wave exclusive prefixes (u16), block scan of the
        // digit totals (thread tid owns digits tid K .. tid K + K - 1)
        uint32_t tot[K], sum = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int d = tid * K + k;
            uint32_t run = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t v = s_wc16[w * RADIX + d];
                s_wc16[w * RADIX + d] = (uint16_t)run;
                run += v;
            }
            tot[k] = run;
            sum += run;
        }
        const uint32_t incl = wave_incl_scan(sum);
        if (lane == 63) s_wsum[wave] = incl;
#pragma unroll
        for (int g = 0; g < G_SCAN; ++g) store_group(G_TOP + G_RANK + g);
        lds_barrier();
        {
            uint32_t pre = 0;
            for (int w = 0; w < wave; ++w) pre += s_wsum[w];
            uint32_t run = pre + incl - sum;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int d = tid * K + k;
                s_start[d] = run;
                s_toff[b][d] -= run;
                run += tot[k];
            }
            if (tid == T - 1) s_start[RADIX] = run;
        }
        lds_barrier();
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const bool valid = dr[i] != ~0u;
            const uint32_t dg = dr[i] & (RADIX - 1);
            const uint32_t sl = valid ? s_start[dg] + s_wc16[wave * RADIX + dg] + (dr[i] >> R) : (uint32_t)TILE;
            s_pos[b][sl] = (uint16_t)(p0 + i * 64);
        }
        const uint32_t cnt = s_start[RADIX];
#pragma unroll
        for (int g = G_TOP + G_RANK + G_SCAN; g < I; ++g) store_group(g);
        pcnt = cnt;
        pP0 = P0;
        lds_barrier();  // staging complete; counters, codes and the previous staging read
        b ^= 1;
    }
    if (walk.first < walk.end) {
#pragma unroll
        for (int g = 0; g < I; ++g) store_group(g);
    }
}

// ---------------------------------------------------------------------------------------------
// Key-range shard select (gk_shard_sort_range)
// ---------------------------------------------------------------------------------------------
// A rank scans the WHOLE sequence and keeps the k-mers whose L0 digit lies in its range -- about
// 1/N of them -- in position order.  One light streaming pass over 4096-position tiles (small LDS
// and registers, so several workgroups per CU overlap their loads): each wave compacts its kept
// k-mers -- the forward 2-bit keys from 8-position windows per lane, the others with one ballot per
// row of 64 positions -- and stores them to consecutive addresses.
// Stable: tiles, waves, rows and lanes follow positions.  The kept k-mers then go through the
// ordinary MSD levels as one bucket (the pass writes their L0 digit bytes, so the first level
// counts 1 byte per k-mer).  A tile is kSR rounds of 4096 positions (512 per wave per round):
// one load of the tile's bytes (or packed words) per kSR rounds keeps more bytes in flight per
// workgroup than one 4096-position tile did.
#ifndef GKM_SEL_ROUNDS
#define GKM_SEL_ROUNDS 1
#endif
constexpr int kST = 512, kSI = 8, kSR = GKM_SEL_ROUNDS;  // threads, rows of 64 positions per wave per round, rounds
constexpr int kSRound = kST * kSI;                       // 4096 positions per round
constexpr int kSTile = kSRound * kSR;                    // positions per tile
constexpr int kSW = kST / 64;                            // waves per tile

// Workgroup w walks its own chunk of tpw consecutive tiles and appends its kept k-mers at a running
// offset into its own region of the output, [t0 * kSTile, (t0 + tpw) * kSTile) (room for every
// position of the chunk, so no count pass is needed); wave_cnt[w] receives the chunk's kept count.
// The regions, in workgroup order, are the pieces of one bucket in position order
// (first_level_from_pieces).
template <int BITS, bool CANON>
#ifndef GKM_SEL_MINW
#define GKM_SEL_MINW 1
#endif
// (tuning override: GKM_SEL_MINW = the waves per SIMD the forward kernels' registers are capped
// for; the canonical ones would spill to scratch)
__global__ __launch_bounds__(kST, CANON ? 1 : GKM_SEL_MINW) void msd0_select_kernel(L0Args a, Dig d0, uint32_t ntiles, uint32_t tpw,
                                                          uint32_t *__restrict__ wave_cnt,
                                                          uint64_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                          uint8_t *__restrict__ nd_out) {
    using P = L0Pack<BITS, kSTile>;
    // per-wave staging of the kept positions (tile-relative u16; the key is re-derived from the
    // tile's codes when it is stored): 512 slots + one dump slot per lane for the positions not
    // kept, so the staging writes need no branch.  (Staged as (key, start), 48 KB, the kernel fit
    // 3 workgroups per CU and its divergent staging loop cost more scalar than vector work.)
    constexpr int kSlots = 512 + 64;
    constexpr int kStage = kSW * kSlots;
    __shared__ uint64_t s_code[P::kCodeWords];
    __shared__ uint32_t s_dol[P::kGroups];
    __shared__ uint8_t s_lut4[256];
    __shared__ uint16_t s_spos[kStage];
    __shared__ uint32_t s_wtot[2][kSW];  // per round parity (a round's barrier orders the reuse)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) s_lut4[tid] = c_code4_msd[tid];
    // tiles of this workgroup: its chunk
    const uint32_t tfirst = blockIdx.x * tpw;
    const uint32_t tend = min(tfirst + tpw, ntiles);
    const uint64_t region = (uint64_t)tfirst * kSTile;  // this chunk's output region
    uint64_t run = 0;                                   // kept so far in the chunk
    uint64_t rr[L0Units<BITS, kSTile, kST>::kPer];
    if (tfirst < tend) l0_load<BITS, kSTile, kST>(a, a.lo + (uint64_t)tfirst * kSTile, rr);
    for (uint32_t t = tfirst; t < tend; ++t) {
        const uint64_t P0 = a.lo + (uint64_t)t * kSTile;
        __syncthreads();  // the LUT; the previous tile's codes and wave totals have been read
        l0_pack<BITS, kSTile, kST>(rr, s_code, s_dol, s_lut4, a.acgt_only, a.pk_code != nullptr);
        __syncthreads();
        // the next tile's bytes fly while this one is processed
        if (t + 1 < tend) l0_load<BITS, kSTile, kST>(a, P0 + (uint64_t)kSTile, rr);
        // the wave's output offset from the kept counts of the tile's waves (block-uniform call)
        auto chunk_offset = [&](uint32_t wcount, int r) -> uint64_t {
            if (lane == 0) s_wtot[r & 1][wave] = wcount;
            __syncthreads();
            uint32_t pre = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < kSW; ++w) {
                const uint32_t v = s_wtot[r & 1][w];
                pre += w < wave ? v : 0u;
                tot += v;
            }
            const uint64_t o = region + run + pre;
            run += tot;
            return o;
        };
        for (int r = 0; r < kSR; ++r) {
            const uint32_t R0 = r * kSRound;                       // the round's first tile position
            // forward 2-bit keys: 8 consecutive positions per thread (Win8).  Canonical keys keep the
            // row layout below (a per-lane loop over the kept positions' canonical keys was slower:
            // 11.9 against 8.3 ms per C5 rank at N = 8)
            if constexpr (BITS == 2 && !CANON) {
                const uint32_t q0 = R0 + tid * 8;
                const Win8 win8 = win8_load(s_code, s_dol, q0);
                uint32_t dig[8];
                const uint32_t keepm = win8_keep(win8, a, d0, (int64_t)a.hi - (int64_t)(P0 + q0), s_dol, q0, dig);
                const uint32_t cnt = (uint32_t)__popc(keepm);
                const uint32_t incl = wave_incl_scan(cnt);
                const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
                const uint64_t o = chunk_offset(total, r);
                // stage the wave's kept positions in position order, then store the k-mers as one
                // coalesced run
                uint16_t *sp = s_spos + wave * kSlots;
                uint32_t j = incl - cnt;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t kp = (keepm >> i) & 1u;
                    sp[kp ? j : 512u + (uint32_t)lane] = (uint16_t)(q0 + i);  // (tile positions < 65,536)
                    j += kp;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
                for (uint32_t e = lane; e < total; e += 64) {
                    const uint32_t p = sp[e];
                    const uint64_t k = l0_key<2>(s_code, p, a.total_bits);
                    kout[o + e] = k;
                    vout[o + e] = (uint32_t)(P0 + p);
                    nd_out[o + e] = (uint8_t)dg_of(k, d0);
                }
            } else {
                // one ballot per row of 64 positions
                const uint32_t wbase = R0 + wave * (kSI * 64);
                uint64_t key[kSI];
                uint32_t at[kSI];
                uint32_t keepm = 0, kept = 0;
#pragma unroll
                for (int i = 0; i < kSI; ++i) {
                    const uint32_t p = wbase + i * 64 + lane;
                    key[i] = l0_key_of<BITS, CANON>(s_code, p, a.total_bits, a.symbols);
                    const bool keep = l0_valid(s_dol, p, a.symbols) && P0 + p < a.hi && l0_owned_key(key[i], a);
                    const uint64_t m = __ballot(keep);
                    at[i] = kept + lanes_below(m);
                    kept += (uint32_t)__popcll(m);
                    keepm |= (keep ? 1u : 0u) << i;
                }
                const uint64_t base = chunk_offset(kept, r);
#pragma unroll
                for (int i = 0; i < kSI; ++i) {
                    if ((keepm >> i) & 1u) {
                        const uint64_t o = base + at[i];
                        kout[o] = key[i];
                        vout[o] = (uint32_t)(P0 + wbase + i * 64 + lane);
                        nd_out[o] = (uint8_t)dg_of(key[i], d0);
                    }
                }
            }
        }  // rounds
    }
    if (tid == 0 && blockIdx.x * tpw < ntiles) wave_cnt[blockIdx.x] = (uint32_t)run;
}

// Key-range select from the packed copy, SWAR (round 6): forward 2-bit keys of <= 32 symbols whose
// sequence has a 2-bit packed copy (a.pk_code / a.pk_dol: 32 positions per u64 of codes and u32 of
// stops).  No LDS tile, no barrier: each WAVE walks its own chunk of gpw consecutive 32-position
// groups, 64 groups (2,048 positions) per step, one group per lane, and appends its kept k-mers at
// a running offset into its own region of the output, [first group * 32, + gpw * 32) -- the pieces
// of one bucket in position order, as the workgroup chunks of msd0_select_kernel are.
// Per lane and group (w = the group's codes, x2 = the top half of the next group's codes):
//   ownership digit of position j = the top own_bits bits of the 32-bit window at bit 2 j of
//   w:x2 (one funnel shift); the range test is one subtract and one compare against the range
//   shifted to the window's top, so the digit is never extracted (~4 VALU per position; the tile
//   select spent ~20 per position, VALU-bound at 2.8 ms per C3 rank);
//   stops: a lane with a stop in its 64-position window smears them over S positions in 5
//   doubling steps (all 32 positions at once).
// The kept positions are staged per wave as group-relative u16 in position order (a loop over the
// set bits of the keep mask), the step's 65 code words beside them, and the k-mers leave as one
// coalesced run: key (re-derived from the staged words), start, L0 digit byte.
constexpr int kRselW = 4;  // waves per workgroup (independent: no barrier)
__global__ __launch_bounds__(kRselW * 64) void msd0_rsel_kernel(L0Args a, Dig d0, uint64_t ngroups, uint64_t gpw,
                                                                 uint32_t lo_w, uint32_t spm1_w,
                                                                 uint32_t *__restrict__ wave_cnt,
                                                                 uint64_t *__restrict__ kout,
                                                                 uint32_t *__restrict__ vout,
                                                                 uint8_t *__restrict__ nd_out) {
    __shared__ uint16_t s_pos[kRselW][2048];
    __shared__ uint64_t s_w[kRselW][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t gw = (uint64_t)blockIdx.x * kRselW + wave;
    const uint64_t g0 = gw * gpw, g1 = min(g0 + gpw, ngroups);
    uint16_t *sp = s_pos[wave];
    uint64_t *sw = s_w[wave];
    const int S = a.symbols, B = a.total_bits;
    uint64_t run = 0;
    const uint64_t out0 = g0 * 32;
    // software pipeline: the next step's words fly while this one is processed
    uint64_t w = 0, w1 = 0;
    uint32_t d = 0, d1 = 0;
    auto load = [&](uint64_t base) {
        const uint64_t g = min(base + (uint64_t)lane, ngroups - 1);
        w = a.pk_code[g];
        w1 = a.pk_code[g + 1];
        d = a.pk_dol[g];
        d1 = a.pk_dol[g + 1];
    };
    if (g0 < g1) load(g0);
    for (uint64_t base = g0; base < g1; base += 64) {
        const uint64_t W0 = w, W1 = w1;
        const uint32_t D0 = d, D1 = d1;
        const bool live = base + (uint64_t)lane < g1;
        if (base + 64 < g1) load(base + 64);
        // ownership: position j <-> bit 31 - j of m (MSB first, the order of the staging loop)
        const uint32_t x0 = (uint32_t)(W0 >> 32), x1 = (uint32_t)W0, x2 = (uint32_t)(W1 >> 32);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int r = (2 * j) & 31;
            const uint32_t hi = j < 16 ? x0 : x1, lo = j < 16 ? x1 : x2;
            const uint32_t win = r ? __builtin_amdgcn_alignbit(hi, lo, 32 - r) : hi;
            m = (m << 1) | (uint32_t)(win - lo_w <= spm1_w);
        }
        // stops: invalid where a stop lies in [j, j + S); D0 / D1 bit 31 - i = position i
        if (__ballot((D0 | D1) != 0)) {
            uint64_t x = ((uint64_t)D0 << 32) | D1;
            uint64_t sm = x;  // sm: a stop in [j, j + len)
            int len = 1;
#pragma unroll
            for (int s = 1; s < 32; s <<= 1) {
                if (2 * len <= S) {
                    sm |= sm << len;
                    len *= 2;
                }
            }
            if (len < S) sm |= sm << (S - len);
            m &= ~(uint32_t)(sm >> 32);
        }
        if (!live) m = 0;
        const uint32_t cnt = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
        if (total == 0) continue;
        // stage: the group-relative positions of the kept k-mers in position order, the words
        uint32_t j = incl - cnt;
        while (m) {
            const uint32_t b = __clz(m);
            sp[j++] = (uint16_t)(lane * 32 + b);
            m ^= 0x80000000u >> b;
        }
        sw[lane] = W0;
        if (lane == 63) sw[64] = W1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        const uint64_t o = out0 + run, P0 = base * 32;
        for (uint32_t e = lane; e < total; e += 64) {
            const uint32_t p = sp[e], q = p >> 5, s = (p & 31) * 2;
            const uint64_t A = sw[q];
            const uint64_t T = s ? (A << s) | (sw[q + 1] >> (64 - s)) : A;
            const uint64_t k = T >> (64 - B);
            kout[o + e] = k;
            vout[o + e] = (uint32_t)(P0 + p);
            nd_out[o + e] = (uint8_t)dg_of(k, d0);
        }
        run += total;
        // the next step's staging overwrites these slots: every lane has read them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    }
    if (lane == 0 && g0 < ngroups) wave_cnt[gw] = (uint32_t)run;
}

// ---------------------------------------------------------------------------------------------
// Key-range ranks' L0, compaction first (round 6): the fused select of msd0_pipe_kernel<..., OWN>
// ranked, staged and keyed EVERY position of the sequence to store the ~1/N it keeps (7.7 ms over
// C3 at any N).  These two kernels test the positions with the SWAR range test of msd0_rsel_kernel
// (forward 2-bit keys of <= 32 symbols, packed copy), compact the kept ones per tile in position
// order, and only then rank, stage and store them -- the L0 partition of the rank's k-mers
// straight from the sequence: no select pass, no 13-byte round trip, no level from pieces.
// Tiles are the L0's (kP0Tile = 768 groups of 32 positions, l0_count's tables); threads < 768
// take one group each in the test, the kept elements then spread over all 1,024 threads in the
// partition's wave-major item order (stable: items of a wave in order, waves in order).
// ---------------------------------------------------------------------------------------------
constexpr int kOwnT = 1024, kOwnG = kP0Tile / 32;  // threads, groups per tile
constexpr int kOwnI = kP0Tile / kOwnT;             // items per thread (capacity: every position)
static_assert(kOwnG <= kOwnT && kOwnI * kOwnT == kP0Tile, "one group per thread; every position fits");

struct OwnTest {
    uint32_t lo_w, spm1_w;  // the range shifted to the top of a 32-bit window (msd0_rsel_kernel)
};

// keep mask of the group at position P (bit 31 - j = position P + j): in [a.lo, a.hi), no stop in
// [j, j + S), ownership digit in range; W0 / W1 / D0 / D1 the group's and the next group's words.
// Wave-uniform call (a ballot inside).
__device__ __forceinline__ uint32_t own_keep(const L0Args &a, OwnTest ot, uint64_t P, uint64_t W0, uint64_t W1,
                                             uint32_t D0, uint32_t D1, bool live) {
    const uint32_t x0 = (uint32_t)(W0 >> 32), x1 = (uint32_t)W0, x2 = (uint32_t)(W1 >> 32);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int r = (2 * j) & 31;
        const uint32_t hi = j < 16 ? x0 : x1, lo = j < 16 ? x1 : x2;
        const uint32_t win = r ? __builtin_amdgcn_alignbit(hi, lo, 32 - r) : hi;
        m = (m << 1) | (uint32_t)(win - ot.lo_w <= ot.spm1_w);
    }
    if (__ballot(live && (D0 | D1) != 0)) {
        uint64_t sm = ((uint64_t)D0 << 32) | D1;
        int len = 1;
#pragma unroll
        for (int s = 1; s < 32; s <<= 1) {
            if (2 * len <= a.symbols) {
                sm |= sm << len;
                len *= 2;
            }
        }
        if (len < a.symbols) sm |= sm << (a.symbols - len);
        m &= ~(uint32_t)(sm >> 32);
    }
    const uint64_t jb = a.lo > P ? a.lo - P : 0, je = a.hi > P ? min(a.hi - P, (uint64_t)32) : 0;
    m &= jb < je ? (uint32_t)((0xFFFFFFFFull >> jb) & ~(0xFFFFFFFFull >> je)) : 0u;
    return live ? m : 0u;
}

// the B-bit key of position j of a group (j in [0, 32))
__device__ __forceinline__ uint64_t group_key(uint64_t W0, uint64_t W1, uint32_t j, int B) {
    const uint32_t s = 2 * j;
    const uint64_t T = s ? (W0 << s) | (W1 >> (64 - s)) : W0;
    return T >> (64 - B);
}

// count pass: per-tile histograms of the kept k-mers' L0 digits (R bits)
template <int R>
__global__ __launch_bounds__(kOwnT) void own_count_kernel(L0Args a, Dig d0, OwnTest ot, uint32_t *__restrict__ tile_hist,
                                                           uint32_t ntiles) {
    constexpr int RADIX = 1 << R, NC = 4;
    __shared__ uint32_t s_hist[RADIX * NC];
    const int t = threadIdx.x;
    const uint64_t g_end = (a.hi + 31) / 32;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int i = t; i < RADIX * NC; i += kOwnT) s_hist[i] = 0;
        __syncthreads();
        if (t < kOwnG) {
            const uint64_t g = a.lo / 32 + (uint64_t)tile * kOwnG + t;
            const bool live = g < g_end;
            const uint64_t gc = live ? g : g_end - 1;
            const uint64_t W0 = a.pk_code[gc], W1 = a.pk_code[gc + 1];
            uint32_t m = own_keep(a, ot, gc * 32, W0, W1, a.pk_dol[gc], a.pk_dol[gc + 1], live);
            while (m) {
                const uint32_t j = __clz(m);
                m ^= 0x80000000u >> j;
                atomicAdd(&s_hist[dg_of(group_key(W0, W1, j, a.total_bits), d0) * NC + (t & (NC - 1))], 1u);
            }
        }
        __syncthreads();
        for (int i = t; i < RADIX; i += kOwnT) {
            uint32_t h = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) h += s_hist[i * NC + c];
            tile_hist[(uint64_t)tile * RADIX + i] = h;
        }
    }
}

// partition pass: the kept k-mers of each tile compacted, ranked by their L0 digit (R bits), staged
// and stored at the tile's digit offsets -- (key, start, next digit) or the packed L0 form (P88)
template <int R, bool P88>
__global__ __launch_bounds__(kOwnT) void own_part_kernel(L0Args a, Dig d0, OwnTest ot,
                                                          const uint32_t *__restrict__ tile_off,
                                                          uint64_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                          uint32_t ntiles, NextDigits nd) {
    constexpr int RADIX = 1 << R, NW = kOwnT / 64;
    __shared__ uint16_t s_pos[kP0Tile];             // kept positions in order, then in digit order
    __shared__ uint64_t s_code[kOwnG + 1];
    __shared__ uint32_t s_wc[NW * RADIX];
    __shared__ uint32_t s_wsum[NW];
    __shared__ uint32_t s_start[RADIX + 1];
    __shared__ uint32_t s_toff[RADIX];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t g_end = (a.hi + 31) / 32;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t g0 = a.lo / 32 + (uint64_t)tile * kOwnG;
        if (t < RADIX) s_toff[t] = tile_off[(uint64_t)tile * RADIX + t];
        uint32_t *wc = s_wc + wave * RADIX;
#pragma unroll
        for (int u = 0; u < (RADIX + 63) / 64; ++u)
            if (u * 64 + lane < RADIX) wc[u * 64 + lane] = 0;
        // 1. test: keep mask and count of this thread's group; its code words into LDS
        uint32_t m = 0;
        if (t < kOwnG) {
            const uint64_t g = g0 + t;
            const bool live = g < g_end;
            const uint64_t gc = live ? g : g_end - 1;
            const uint64_t W0 = a.pk_code[gc], W1 = a.pk_code[gc + 1];
            m = own_keep(a, ot, gc * 32, W0, W1, a.pk_dol[gc], a.pk_dol[gc + 1], live);
            s_code[t] = W0;
            if (t == kOwnG - 1) s_code[kOwnG] = W1;
        }
        const uint32_t cnt = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan(cnt);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t pre = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t v = s_wsum[w];
            pre += w < wave ? v : 0u;
            total += v;
        }
        // 2. compaction: the kept positions (tile-relative) in position order
        {
            uint32_t j = pre + incl - cnt;
            while (m) {
                const uint32_t b = __clz(m);
                m ^= 0x80000000u >> b;
                s_pos[j++] = (uint16_t)(t * 32 + b);
            }
        }
        __syncthreads();
        // 3. rank: element e = wave * kOwnI * 64 + i * 64 + lane (wave-major, position order)
        uint32_t dr[kOwnI];
        uint16_t pp[kOwnI];
        const uint32_t e0 = wave * (kOwnI * 64);
#pragma unroll
        for (int i = 0; i < kOwnI; ++i) {
            dr[i] = ~0u;
            pp[i] = 0;
            if (e0 + i * 64 < total) {  // (wave-uniform)
                const uint32_t e = e0 + i * 64 + lane;
                const bool valid = e < total;
                const uint32_t p = s_pos[valid ? e : 0];
                const uint32_t dig = dg_of(l0_key<2>(s_code, p, a.total_bits), d0);
                const uint32_t rk = rank_atomic(wc, dig, valid);
                dr[i] = valid ? dig | (rk << 8) : ~0u;
                pp[i] = (uint16_t)p;
            }
        }
        __syncthreads();  // ranks final; every compacted position read
        // 4. digit starts: per-digit totals over the waves, their scan
        uint32_t dtot = 0, dincl = 0;
        if (t < RADIX) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t v = s_wc[w * RADIX + t];
                s_wc[w * RADIX + t] = dtot;
                dtot += v;
            }
            dincl = wave_incl_scan(dtot);
            if (lane == 63) s_wsum[wave] = dincl;
        }
        __syncthreads();
        if (t < RADIX) {
            uint32_t p2 = 0;
            for (int w = 0; w < wave; ++w) p2 += s_wsum[w];
            const uint32_t st = p2 + dincl - dtot;
            s_start[t] = st;
            s_toff[t] -= st;
        }
        __syncthreads();
        // 5. stage in digit order (over the compacted positions: all were read in 3)
#pragma unroll
        for (int i = 0; i < kOwnI; ++i) {
            if (dr[i] != ~0u) {
                const uint32_t dg = dr[i] & 0xFFu;
                s_pos[s_start[dg] + wc[dg] + (dr[i] >> 8)] = pp[i];
            }
        }
        __syncthreads();
        // 6. store: runs of each digit at the tile's offsets
        const uint64_t P0 = g0 * 32;
        for (uint32_t s = t; s < total; s += kOwnT) {
            const uint32_t p = s_pos[s];
            const uint64_t key = l0_key<2>(s_code, p, a.total_bits);
            const uint64_t o = (uint64_t)s_toff[dg_of(key, d0)] + s;
            const uint32_t st = (uint32_t)(P0 + p);
            if (P88) {
                const int shi = nd.pshi;
                kout[o] = (key << shi) | (st >> (32 - shi));
                nd.out16[o] = (uint16_t)(st & ((1u << (32 - shi)) - 1));
            } else {
                kout[o] = key;
                vout[o] = st;
            }
            nd.out[o] = (uint8_t)dg_of(key, nd.d);
        }
        __syncthreads();  // the staging and the codes are read before the next tile's
    }
}

// The same histogram from the packed copy, SWAR (round 6; forward 2-bit keys of <= 32 symbols, as
// msd0_rsel_kernel): one 32-position group per lane, the digit of position j the top own_bits bits
// of the 32-bit window at bit 2 j of the group's codes; positions that start no k-mer (a stop in
// [j, j + S), or outside [lo, hi)) count into junk bins (4096 + 64 j + lane: conflict-free) instead
// of being branched around.  One LDS table per workgroup, its waves walking the chunk together.
__global__ __launch_bounds__(kRselW * 64) void own_hist_rsel_kernel(L0Args a, uint64_t gpb,
                                                                     uint32_t *__restrict__ ghist) {
    __shared__ uint32_t s_hist[4096 + 64 * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 4096 + 64 * 32; i += kRselW * 64) s_hist[i] = 0;
    __syncthreads();
    const uint64_t G0 = a.lo / 32, G1 = (a.hi + 31) / 32;
    const uint64_t g0 = G0 + blockIdx.x * gpb, g1 = min(g0 + gpb, G1);
    const int S = a.symbols, osh = 32 - a.own_bits;
    for (uint64_t base = g0 + wave * 64; base < g1; base += kRselW * 64) {
        const uint64_t g = base + lane;
        const bool live = g < g1;
        const uint64_t gc = live ? g : g1 - 1;
        const uint64_t W0 = a.pk_code[gc], W1 = a.pk_code[gc + 1];
        const uint32_t D0 = a.pk_dol[gc], D1 = a.pk_dol[gc + 1];
        // valid positions, bit 31 - j = position j: inside [lo, hi) ...
        const uint64_t P0 = gc * 32;
        const uint64_t jb = a.lo > P0 ? a.lo - P0 : 0, je = a.hi - P0 < 32 ? a.hi - P0 : 32;
        uint32_t m = live && jb < je ? (uint32_t)((0xFFFFFFFFull >> jb) & ~(0xFFFFFFFFull >> je)) : 0u;
        // ... and no stop in [j, j + S)
        if (__ballot((D0 | D1) != 0)) {
            uint64_t sm = ((uint64_t)D0 << 32) | D1;
            int len = 1;
#pragma unroll
            for (int s = 1; s < 32; s <<= 1) {
                if (2 * len <= S) {
                    sm |= sm << len;
                    len *= 2;
                }
            }
            if (len < S) sm |= sm << (S - len);
            m &= ~(uint32_t)(sm >> 32);
        }
        const uint32_t x0 = (uint32_t)(W0 >> 32), x1 = (uint32_t)W0, x2 = (uint32_t)(W1 >> 32), inv = ~m;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int r = (2 * j) & 31;
            const uint32_t hi = j < 16 ? x0 : x1, lo = j < 16 ? x1 : x2;
            const uint32_t win = r ? __builtin_amdgcn_alignbit(hi, lo, 32 - r) : hi;
            // (an invalid position's bin depends on the lane only: the N runs of a mixed sba would
            // otherwise send a whole wave to one address, serialising the atomic)
            const uint32_t bin = ((inv >> (31 - j)) & 1u) ? 4096u + 64u * j + (uint32_t)lane : win >> osh;
            atomicAdd(&s_hist[bin], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << a.own_bits); i += kRselW * 64)
        if (s_hist[i]) atomicAdd(&ghist[i], s_hist[i]);
}

// Ownership-digit histogram of a key-range shard's position share: the top own_bits (<= 12) bits
// of every k-mer starting in [a.lo, a.hi), one LDS table per workgroup flushed into ghist.
template <int BITS, bool CANON>
__global__ __launch_bounds__(kST) void own_hist_kernel(L0Args a, uint32_t ntiles, uint32_t *__restrict__ ghist) {
    using P = L0Pack<BITS, kSTile>;
    __shared__ uint64_t s_code[P::kCodeWords];
    __shared__ uint32_t s_dol[P::kGroups];
    __shared__ uint8_t s_lut4[256];
    __shared__ uint32_t s_hist[4096];
    const int tid = threadIdx.x;
    if (tid < 256) s_lut4[tid] = c_code4_msd[tid];
    for (int i = tid; i < 4096; i += kST) s_hist[i] = 0;
    const int osh = a.total_bits - a.own_bits;
    uint64_t rr[L0Units<BITS, kSTile, kST>::kPer];
    if (blockIdx.x < ntiles) l0_load<BITS, kSTile, kST>(a, a.lo + (uint64_t)blockIdx.x * kSTile, rr);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t P0 = a.lo + (uint64_t)t * kSTile;
        __syncthreads();  // the LUT and the zeroed table; the previous tile's codes have been read
        l0_pack<BITS, kSTile, kST>(rr, s_code, s_dol, s_lut4, a.acgt_only, a.pk_code != nullptr);
        __syncthreads();
        if (t + gridDim.x < ntiles) l0_load<BITS, kSTile, kST>(a, P0 + (uint64_t)gridDim.x * kSTile, rr);
#pragma unroll
        for (int i = 0; i < kSI * kSR; ++i) {
            const uint32_t p = i * kST + tid;
            const uint64_t key = l0_key_of<BITS, CANON>(s_code, p, a.total_bits, a.symbols);
            if (l0_valid(s_dol, p, a.symbols) && P0 + p < a.hi) atomicAdd(&s_hist[(uint32_t)(key >> osh)], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < (1 << a.own_bits); i += kST)
        if (s_hist[i]) atomicAdd(&ghist[i], s_hist[i]);
}

// ---------------------------------------------------------------------------------------------
// 2-bit packed copy of an ACGT sba: one u64 of codes (A0 C1 G2 T3, MSB first) and one u32 stop
// mask ('$') per 32 positions -- the layout the L0 kernels build in LDS.  Packed once per sort and
// read by every full-sequence pass (L0 count and partition; histogram, select count and store of
// the key-range shards) instead of each pass re-packing the bytes: 0.28 B per position.
// ---------------------------------------------------------------------------------------------
template <bool NONACGT = false>
__global__ __launch_bounds__(256) void pack2_kernel(const uint8_t *__restrict__ sba, uint64_t nwords,
                                                    uint64_t *__restrict__ code, uint32_t *__restrict__ dol) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < nwords; g += (uint64_t)gridDim.x * 256) {
        uint64_t cw;
        uint32_t dw;
        pack2_word<NONACGT>(sba + 32 * g, cw, dw);
        code[g] = cw;
        dol[g] = dw;
    }
}

// starts-only shards (GK_SHARD_STARTS_ONLY): key of the k-mer at every received start from the 2-bit
// packed copy (B <= 64 bits: the first word), and its next-level digit byte
__global__ __launch_bounds__(256) void keys_from_starts_kernel(const uint64_t *__restrict__ pk,
                                                                const uint32_t *__restrict__ vin, uint64_t n, int B,
                                                                Dig dn, uint64_t *__restrict__ kout,
                                                                uint8_t *__restrict__ nd) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t s = vin[i], q = s >> 5, sh = (s & 31) * 2;
        const uint64_t A = pk[q];
        const uint64_t T = sh ? (A << sh) | (pk[q + 1] >> (64 - sh)) : A;
        const uint64_t key = T >> (64 - B);
        kout[i] = key;
        nd[i] = (uint8_t)dg_of(key, dn);
    }
}

}  // namespace gkm
