// gkm_msd_local.h -- the local rounds of the MSD sort: buckets of <= kBlockMax elements finished
// in LDS, one workgroup (msd_local_kernel), one wave (msd_wave_kernel) or one thread
// (msd_tiny_kernel) per bucket.
// Private to gkm_msd.hip.  Needs gkm_msd_config.h and gkm_msd_lists.h (Lists, route, compact_key).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkm_msd_config.h"
#include "gkm_msd_lists.h"
#include "gkm_partition.h"

namespace gkm {

// ---------------------------------------------------------------------------------------------
// local rounds: a bucket of <= T*I elements per workgroup, persistent over a list
// ---------------------------------------------------------------------------------------------
// Per bucket (entry = start, len, hi, parity):
//   1. stable partition by the R-bit digit below the top `hi` bits into LDS (partition_stage);
//   2. each sub-bucket: singleton, or no key bits left after this digit (equal keys, already in
//      start order) -> final; <= kSmall -> rank-by-count on the key (ties: staging order =
//      start order); larger -> left in stable order and re-listed for the next round (its head
//      flags are provisional: that round rewrites them);
//   3. keys, starts and head flags (key differs from its predecessor) are written back in order.
// Output always goes to buffer 0; the bucket is read fully before any write, so in place is safe.
// Loads and stores are branch-free with static counts (clamped to the bucket), so the next
// bucket's loads -- issued once the current one is final in LDS -- overlap its stores.
// Common-prefix skip: x_or = OR over a bucket's keys of (key ^ first key).  The bits of the key
// below the hi sorted ones that are equal in every element need no partition pass: the bucket's
// next digit starts at its highest differing bit.  All keys equal: one last digit (one sub-bucket,
// final).  Repeats make such buckets common (a 30-copy repeat k-mer would otherwise take one round
// per 8 bits).
__device__ __forceinline__ int skip_hi(uint64_t x_or, int B, int hi) {
    const int rem = B - hi;
    if (rem <= 0) return hi;
    x_or &= rem >= 64 ? ~0ull : ((1ull << rem) - 1);
    if (x_or == 0) return max(hi, B - 8);
    return B - 1 - (63 - __clzll(x_or));
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x |= __shfl_xor(x, off);
    return x;
}

// compact inputs (first local round after a compact level): where to find the elements' low key
// bits and next digits, and the entries' prefixes
struct CompactIn {
    const uint64_t *pref;  // per list entry (null: no entry is compact)
    const uint8_t *nd;
};

template <int T, int I>
__device__ __forceinline__ void local_load(const uint2 e, const uint64_t *k0, const uint32_t *v0, const uint64_t *k1,
                                           const uint32_t *v1, uint64_t (&key)[I], uint32_t (&val)[I],
                                           uint64_t pf = 0, const CompactIn *ci = nullptr, int B = 0) {
    const uint64_t st = e.x;
    const uint32_t len = e.y >> 8;
    const uint64_t *sk = (e.y & 1) ? k1 : k0;
    const uint32_t *sv = (e.y & 1) ? v1 : v0;
    uint32_t q0 = (threadIdx.x >> 6) * (I * 64) + (threadIdx.x & 63);
    asm volatile("" : "+v"(q0));
    if (pf & kCompact) {  // (uniform: one bucket per wave / workgroup)
        const int hi = (e.y >> 1) & 127;
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const uint64_t e_ = st + min(q0 + i * 64, len - 1);
            const uint64_t x = sk[e_];
            key[i] = compact_key(pf, hi, B, ci->nd[e_], (uint32_t)(x >> 32));
            val[i] = (uint32_t)x;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < I; ++i) {
        const uint64_t e_ = st + min(q0 + i * 64, len - 1);
        key[i] = sk[e_];
        val[i] = sv[e_];
    }
}

template <int T, int I, int R>
__global__ __launch_bounds__(T) void msd_local_kernel(const uint2 *__restrict__ list, uint32_t count, int B,
                                                      uint64_t *k0, uint32_t *v0, const uint64_t *k1,
                                                      const uint32_t *v1, uint8_t *__restrict__ heads, Lists L,
                                                      uint32_t *__restrict__ ctr, int skip, uint32_t small, int wkeys,
                                                      CompactIn ci) {
    using SM = PartSmem<T, I, R>;
    constexpr int TILE = SM::kTile;
    constexpr int RADIX = SM::kRadix;
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[SM::kUnion];
    __shared__ uint32_t s_wsum[SM::kWaves];
    __shared__ uint32_t s_start[RADIX + 1];
    __shared__ uint8_t s_hd[TILE + 1];
    __shared__ uint32_t s_any;
    __shared__ uint64_t s_kf, s_or;                  // common-prefix skip: first key, OR of differences
    uint64_t *s_k = reinterpret_cast<uint64_t *>(s_raw);
    uint32_t *s_v = reinterpret_cast<uint32_t *>(s_raw + SM::kValOff);
    uint32_t *s_wc = reinterpret_cast<uint32_t *>(s_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t idx = blockIdx.x;
    if (idx >= count) return;
    uint2 e = list[idx];
    uint64_t pf = ci.pref ? ci.pref[idx] : 0;
    uint64_t key[I];
    uint32_t val[I];
    local_load<T, I>(e, k0, v0, k1, v1, key, val, pf, &ci, B);
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    for (; idx < count; idx += gridDim.x) {
        const uint2 ce = e;
        const uint64_t st = ce.x;
        const uint32_t len = ce.y >> 8;
        int hi = (ce.y >> 1) & 127;
        if (skip) {
            if (tid == 0) {
                s_kf = key[0];
                s_or = 0;
            }
            lds_barrier();
            uint64_t x = 0;
#pragma unroll
            for (int i = 0; i < I; ++i)
                if ((uint32_t)(wave * (I * 64) + i * 64 + lane) < len) x |= key[i] ^ s_kf;
            x = wave_or64(x);
            if (lane == 0 && x) atomicOr((unsigned long long *)&s_or, (unsigned long long)x);
            lds_barrier();
            hi = skip_hi(s_or, B, hi);
        }
        const Dig dd = dig_at(B, hi, R);
        const int nhi = hi + R;      // key bits sorted within a sub-bucket
        const bool last = nhi >= B;  // sub-bucket keys are equal
        if (idx + gridDim.x < count) {  // else: re-load the current one
            e = list[idx + gridDim.x];
            pf = ci.pref ? ci.pref[idx + gridDim.x] : 0;
        }

        // 1. stable partition into LDS
        for (int i = tid; i < SM::kWaves * RADIX; i += T) s_wc[i] = 0;
        if (tid == 0) s_any = 0;
        lds_barrier();
        bool valid[I];
        uint32_t slot[I];
#pragma unroll
        for (int i = 0; i < I; ++i) valid[i] = (uint32_t)(wave * (I * 64) + i * 64 + lane) < len;
        // items of this wave holding elements (wave-uniform)
        const int wbase = wave * (I * 64);
        const int live = (int)len > wbase ? min(I, ((int)len - wbase + 63) >> 6) : 0;
        partition_stage<T, I, R>(key, val, valid, dd, s_raw, nullptr, s_wsum, s_start, slot, nullptr, live);

        // 2. final position and head flag of every element
        uint32_t out[I];
        uint8_t hd[I];
#pragma unroll
        for (int i = 0; i < I; ++i) {
            out[i] = slot[i];
            hd[i] = 0;
            if (i >= live) continue;  // wave-uniform
            const uint32_t dg = dg_of(key[i], dd);
            const uint32_t sb = s_start[dg], size = s_start[dg + 1] - sb;
            hd[i] = slot[i] == sb;  // singleton or equal keys: the first is the head
            if (valid[i] && size > 1 && !last) {
                if (size <= small) {
                    const uint32_t me = slot[i] - sb;
                    uint32_t lt = 0, eq = 0;
                    for (uint32_t j = 0; j < size; ++j) {
                        const uint64_t kj = s_k[sb + j];
                        lt += kj < key[i];
                        eq += kj == key[i] && j < me;
                    }
                    out[i] = sb + lt + eq;
                    hd[i] = eq == 0;
                } else {
                    hd[i] = 2;  // not final: re-listed, head written by the next round
                }
            }
        }
        // re-list the large sub-buckets (rare): one entry each, from its first element
        bool first[I], any = false;
#pragma unroll
        for (int i = 0; i < I; ++i) {
            first[i] = valid[i] && hd[i] == 2 && slot[i] == s_start[dg_of(key[i], dd)];
            any |= first[i];
        }
        if (any) s_any = 1;
        lds_barrier();  // also: every rank-by-count read is done before the staging is overwritten
        const bool relist = s_any != 0;
        if (relist) {
#pragma unroll
            for (int i = 0; i < I; ++i) {
                const uint32_t dg = dg_of(key[i], dd);
                const uint32_t size = first[i] ? s_start[dg + 1] - s_start[dg] : 0;
                route((uint32_t)st + slot[i], size, nhi, B, 0, false, L, ctr, lane);
            }
        }
#pragma unroll
        for (int i = 0; i < I; ++i) {  // invalid items: out = sink slot
            if (i >= live) continue;
            s_k[out[i]] = key[i];
            s_v[out[i]] = val[i];
            s_hd[out[i]] = hd[i];  // 0 / 1: final (not) a group head; 2: re-listed
        }
        // the next bucket's loads fly while this one is written back
        local_load<T, I>(e, k0, v0, k1, v1, key, val, pf, &ci, B);  // unconditional: static load count
        lds_barrier();

        // 3. in-order write-back with head flags
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const uint32_t p = min((uint32_t)(i * T + tid), len - 1);
            if (relist || wkeys) k0[st + p] = s_k[p];  // keys: final-key sorts, or re-listed elements
            v0[st + p] = s_v[p];
            heads[st + p] = s_hd[p] & 1;
        }
        lds_barrier();  // the write-back has read LDS before the next bucket's staging
    }
}

// list entry j of a wave class (scalar loads) and its prefix (0: not recorded)
__device__ __forceinline__ void wave_entry(const uint2 *__restrict__ list, const uint64_t *__restrict__ cpref,
                                           uint32_t j, uint2 &e, uint64_t &pf) {
    e = list[j];
    pf = cpref ? cpref[j] : 0ull;
}

// raw elements of a wave-class bucket: compact (x = low << 32 | start, next-digit byte) or full
// (key, start).  One global load instruction per word either way (so the compiler's count of
// loads in flight is static); buffers chosen by integer selects (pointer selects between kernel
// arguments went through the stack as flat loads).  Loads clamped to the bucket.
template <int I>
__device__ __forceinline__ void wave_load(const uint2 e, uint64_t pf, int lane, const uint64_t *k0, const uint64_t *k1,
                                          const uint32_t *v0, const uint32_t *v1, const uint8_t *cnd,
                                          uint64_t (&a)[I], uint32_t (&b)[I]) {
    const uint64_t st = e.x;
    const uint32_t len = e.y >> 8;
    const bool p1 = (e.y & 1) != 0, cmp = (pf & kCompact) != 0;
    const uint64_t kb = p1 ? (uint64_t)k1 : (uint64_t)k0;
    const uint64_t bb = cmp ? (uint64_t)cnd : (p1 ? (uint64_t)v1 : (uint64_t)v0);
    const int sh = cmp ? 0 : 2;
    uint32_t q = lane;
    asm volatile("" : "+v"(q));
    if (cmp) {  // byte loads of the digits: 0.1-0.3 ms faster than unaligned 4-byte ones at C3 (A/B)
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const uint64_t at = st + min(q + i * 64, len - 1);
            a[i] = *reinterpret_cast<gu64 *>(kb + 8 * at);
            b[i] = *reinterpret_cast<gu8 *>(bb + at);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < I; ++i) {
        const uint64_t at = st + min(q + i * 64, len - 1);
        a[i] = *reinterpret_cast<gu64 *>(kb + 8 * at);
        b[i] = *reinterpret_cast<gu32u *>(bb + (at << sh));
    }
}

// Single-wave finishing kernel for buckets of <= 64 I elements (C3: ~370 keys behind the compact
// level, class 1).  Per bucket, one wave:
//   keys   compact entries (a compact level's output): key = prefix | next-digit byte | low bits
//          (compact_key); full entries: (key, start) as stored
//   rank   the next 8-bit digit of every element, ranked by ONE returning LDS atomic per item
//          (rank_atomic: stable); the 256 digit counts are scanned 4 per lane (wave_incl_scan)
//   order  each digit's elements take its slots in stable order; the key bits below the digit are
//          staged at those slots, and a sub-bucket of 2..small elements is ordered by
//          rank-by-count over them (ties: staging order = start order); larger sub-buckets are
//          re-listed for another round; a sub-bucket whose key bits are exhausted is final
//   write  keys (the group-head flag in bit 63 when B < 64) and starts staged at their final slots,
//          then stored contiguously: keys, starts and head flags of the whole bucket
// The next bucket's elements are loaded once the current one is staged in LDS, so they fly during
// its write-back; loads and write-back are branch-free with static counts (slots clamped to the
// bucket), so the next iteration waits for those loads without draining the stores.  The list entries and prefixes are scalar loads two
// buckets ahead.  LDS per wave: staged keys (aliased by the low bits of the ranking: one wave's LDS
// operations complete in order), staged starts, digit counts -- 7.2 KB at I = 8.
// WK: keys are written back (one-word sorts); otherwise only for buckets with re-listed elements.
template <int I, int MINW, bool WK, int R>
__global__ __launch_bounds__(64, MINW) void msd_wave_kernel(const uint2 *__restrict__ list, uint32_t count, int B,
                                                      uint64_t *k0, uint32_t *v0, const uint64_t *k1,
                                                      const uint32_t *v1, uint8_t *__restrict__ heads,
                                                      const Lists *__restrict__ Lp, uint32_t *__restrict__ ctr,
                                                      int skip, uint32_t small, const uint64_t *__restrict__ cpref,
                                                      const uint8_t *__restrict__ cnd) {
    constexpr int CAP = 64 * I;
    // bit budget of the packed per-item words below: sub-bucket start (slot) in 10 bits, size in 11,
    // rank in 11, and the slot in the low 10 bits of a composite rank-by-count value
    static_assert(CAP <= 1024, "slot fields are 10 bits wide");
    constexpr int MINLIVE = I > 4 ? I / 2 + 1 : 1;  // items a bucket of the class always fills
    constexpr int RADIX = 1 << R, CPL = RADIX / 64;  // digits; counters per lane in the scan
    static_assert(CPL % 4 == 0, "16-byte counter groups");
    __shared__ uint64_t s_k[CAP + 4];  // staged keys (slot CAP: sink); rank-by-count values + sentinels
    // digit counts -> starts (s_cnt[RADIX] = len); once the ranks are final, the staged starts
    // (slot CAP: sink) -- one wave's LDS operations complete in order
    constexpr int kUnion = (RADIX + 4) > (CAP + 1) ? (RADIX + 4) : (CAP + 1);
    __shared__ __attribute__((aligned(16))) uint32_t s_cv[kUnion];
    uint32_t *const s_cnt = s_cv;
    uint32_t *const s_v = s_cv;
    const int lane = threadIdx.x;
    // XCD-aware walk (grid a multiple of 8): workgroup b takes the (b % 8)-th eighth of the list,
    // so the list's neighbouring buckets -- neighbours in memory, since classify appends a level's
    // sub-buckets in runs of address order -- are finished at about the same time on one XCD and
    // share the L2 lines at their edges; other grids walk the list with the plain stride
    uint32_t idx = blockIdx.x, lend = count, lstep = gridDim.x;
    if (gridDim.x >= 8 && (gridDim.x & 7) == 0) {
        const uint32_t x = blockIdx.x & 7;
        idx = (uint32_t)((uint64_t)count * x / 8) + (blockIdx.x >> 3);
        lend = (uint32_t)((uint64_t)count * (x + 1) / 8);
        lstep = gridDim.x >> 3;
    }
    if (idx >= lend) return;
    // keys and starts of a bucket from its raw elements
    auto unpack = [B](const uint2 e, uint64_t pf, const uint64_t (&a)[I], const uint32_t (&b)[I], uint64_t (&key)[I],
                      uint32_t (&val)[I]) {
        const int hi0 = (e.y >> 1) & 127;
        const bool cmp = (pf & kCompact) != 0;
#pragma unroll
        for (int i = 0; i < I; ++i) {
            key[i] = cmp ? compact_key(pf, hi0, B, b[i] & 0xFFu, (uint32_t)(a[i] >> 32)) : a[i];
            val[i] = cmp ? (uint32_t)a[i] : b[i];
        }
    };
    uint2 e, en;
    uint64_t pf, pfn;
    uint64_t key[I], a[I];
    uint32_t val[I], b[I];
    wave_entry(list, cpref, idx, e, pf);
    wave_load<I>(e, pf, lane, k0, k1, v0, v1, cnd, a, b);
    en = e;
    pfn = pf;
    if (idx + lstep < lend) wave_entry(list, cpref, idx + lstep, en, pfn);
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    for (;;) {
        const uint64_t st = e.x;
        const uint32_t len = e.y >> 8;
        const int hi0 = (e.y >> 1) & 127;
        unpack(e, pf, a, b, key, val);
        uint2 enn = en;
        uint64_t pfnn = pfn;
        if (idx + 2 * lstep < lend) wave_entry(list, cpref, idx + 2 * lstep, enn, pfnn);

        int hi = hi0;
        if (skip) {  // common-prefix skip (later rounds and phases: repeats)
            const uint64_t kf = ((uint64_t)__builtin_amdgcn_readlane((int)(uint32_t)(key[0] >> 32), 0) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key[0], 0);
            uint64_t x = 0;
#pragma unroll
            for (int i = 0; i < I; ++i)
                if ((uint32_t)(i * 64 + lane) < len) x |= key[i] ^ kf;
            hi = skip_hi(wave_or64(x), B, hi);
        }
        const Dig dd = dig_at(B, hi, R);
        const bool last = hi + R >= B;                      // a sub-bucket's keys are equal
        const uint64_t lowm = (1ull << dd.shift) - 1ull;    // key bits below the digit
        const int live = min(I, (int)((len + 63) >> 6));    // items holding elements (wave-uniform)

        // 1. stable rank inside the digit
#pragma unroll
        for (int u = 0; u < CPL / 4; ++u) reinterpret_cast<uint4 *>(s_cnt)[lane * (CPL / 4) + u] = make_uint4(0, 0, 0, 0);
        uint32_t pk[I];  // rank | digit << 16, then rank << 21 | size << 10 | sub-bucket start
#pragma unroll
        for (int i = 0; i < I; ++i) {
            pk[i] = 0;
            if (i >= live) continue;
            const uint32_t d = dg_of(key[i], dd);
            pk[i] = rank_atomic(s_cnt, d, (uint32_t)(i * 64 + lane) < len) | (d << 16);
        }
        // 2. digit starts (exclusive scan of the RADIX counts, CPL per lane); s_cnt[RADIX] = len
        {
            uint4 c[CPL / 4];
            uint32_t sl = 0;
#pragma unroll
            for (int u = 0; u < CPL / 4; ++u) {
                c[u] = reinterpret_cast<const uint4 *>(s_cnt)[lane * (CPL / 4) + u];
                sl += c[u].x + c[u].y + c[u].z + c[u].w;
            }
            const uint32_t incl = wave_incl_scan(sl);
            uint32_t r0 = incl - sl;
#pragma unroll
            for (int u = 0; u < CPL / 4; ++u) {
                const uint4 o = make_uint4(r0, r0 + c[u].x, r0 + c[u].x + c[u].y, r0 + c[u].x + c[u].y + c[u].z);
                reinterpret_cast<uint4 *>(s_cnt)[lane * (CPL / 4) + u] = o;
                r0 = o.w + c[u].w;
            }
            if (lane == 63) s_cnt[RADIX] = incl;
        }
        // 3. slots.  Staged at each element's slot: its key bits below the sorted ones (digit and
        // low bits) with the slot appended -- (x << 10) | slot, unique, and in sub-bucket order
        // exactly the stable order -- when they fit 64 bits; otherwise the low bits alone.  Four
        // sentinels (all ones) follow the bucket, so a rank-by-count may read past its sub-bucket
        // unpredicated: later digits and sentinels are larger than any of its values.
        const bool cmpst = hi + 64 - 10 >= B;  // composite values (C3: 39 + 10 bits)
        const uint64_t xm = B - hi >= 64 ? ~0ull : (1ull << (B - hi)) - 1ull;
#pragma unroll
        for (int i = 0; i < I; ++i) {
            if (i >= live) continue;
            const uint32_t d = pk[i] >> 16, r = pk[i] & 0xFFFFu;
            const uint32_t sb = s_cnt[d], size = s_cnt[d + 1] - sb;
            if ((uint32_t)(i * 64 + lane) < len)
                s_k[sb + r] = cmpst ? ((key[i] & xm) << 10) | (sb + r) : key[i] & lowm;
            pk[i] = (r << 21) | (size << 10) | sb;
        }
        if (lane < 4) s_k[len + lane] = ~0ull;
        // 4. final slot of every element: sub-buckets of 2..small elements by rank-by-count
        bool any = false;
#pragma unroll
        for (int i = 0; i < I; ++i) {
            if (i >= live) continue;
            const uint32_t sb = pk[i] & 0x3FFu, size = (pk[i] >> 10) & 0x7FFu, r = pk[i] >> 21;
            const bool valid = (uint32_t)(i * 64 + lane) < len;
            uint32_t o = valid ? sb + r : (uint32_t)CAP;  // invalid items: the sink
            any |= valid && size > small && !last;        // re-listed: ordered by the next round
            if (valid && size > 1 && size <= small && !last) {
                uint32_t cnt = 0;
                if (cmpst) {
                    const uint64_t me = ((key[i] & xm) << 10) | (sb + r);
                    for (uint32_t j0 = 0; j0 < size; j0 += 4) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) cnt += s_k[sb + j0 + u] < me;
                    }
                } else {  // low bits; ties by slot
                    const uint64_t me = key[i] & lowm;
                    uint32_t lt = 0, eq = 0;
                    for (uint32_t j0 = 0; j0 < size; j0 += 4) {
                        uint64_t x[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) x[u] = s_k[sb + j0 + u];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const uint32_t j = j0 + u;
                            lt += (j < size) & (x[u] < me);
                            eq += (j < r) & (x[u] == me);
                        }
                    }
                    cnt = lt + eq;
                }
                o = sb + cnt;
            }
            pk[i] = o;
        }
        const bool relist = __ballot(any) != 0;
        if (relist) {  // (rare) one entry per re-listed sub-bucket, from its first element
#pragma unroll
            for (int i = 0; i < I; ++i) {
                uint32_t size = 0, at = 0;
                if (i < live && (uint32_t)(i * 64 + lane) < len) {
                    const uint32_t d = dg_of(key[i], dd);
                    const uint32_t sb = s_cnt[d];
                    size = s_cnt[d + 1] - sb;
                    at = pk[i];
                    if (size <= small || last || at != sb) size = 0;
                }
                route((uint32_t)st + at, size, hi + R, B, 0, false, *Lp, ctr, lane);
            }
        }
        // 5. stage at the final slots (after every rank-by-count read of s_k: in order)
#pragma unroll
        for (int i = 0; i < I; ++i) {
            if (i >= live) continue;
            s_k[pk[i]] = key[i];
            s_v[pk[i]] = val[i];
        }
        // the next bucket's raw elements (after the last: this one again -- a static count): its
        // keys and starts are staged, so their registers take the loads, which fly during the
        // write-back (loading at the top of the bucket instead kept two buckets in registers:
        // 4 waves per SIMD, measured 22.2 against 20.3 ms at C3)
        wave_load<I>(en, pfn, lane, k0, k1, v0, v1, cnd, a, b);
        // 6. write-back: contiguous; group-head flag = the key differs from its predecessor (a
        // bucket starts a group; re-listed elements get provisional flags).  Items that may be
        // empty first, skipped when they are; then the MINLIVE items every bucket of the class
        // fills (its buckets hold more than CAP / 2 elements), unconditionally: the compiler then
        // knows at least 3 MINLIVE stores follow the next bucket's loads, and the next iteration
        // waits for those loads without draining them (a branch around every item's stores
        // drained all; stores for empty items cost more than the drain)
        const bool wk = WK || relist;
#pragma unroll
        for (int ii = 0; ii < I; ++ii) {
            const int i = ii < I - MINLIVE ? MINLIVE + ii : ii - (I - MINLIVE);
            if (i >= MINLIVE && i >= live) continue;
            const uint32_t j = min((uint32_t)(i * 64 + lane), len - 1);
            const uint64_t kj = s_k[j], kp = s_k[j > 0 ? j - 1 : 0];
            const uint32_t vj = s_v[j];
            if (wk) gmem(k0)[st + j] = kj;
            gmem(v0)[st + j] = vj;
            gmem(heads)[st + j] = (j == 0 || kj != kp) ? 1 : 0;
        }
        idx += lstep;
        if (idx >= lend) break;
        e = en;
        pf = pfn;
        en = enn;
        pfn = pfnn;
    }
}

// Buckets of <= kTiny elements (mostly from the tie groups of multi-word keys): one thread per
// bucket, stable rank-by-count over the full word (ties: load order = start order), write-back of
// starts and head flags to buffer 0.
__global__ __launch_bounds__(256) void msd_tiny_kernel(const uint2 *__restrict__ list, uint32_t count,
                                                       uint64_t *k0, uint32_t *v0, const uint64_t *k1,
                                                       const uint32_t *v1, uint8_t *__restrict__ heads, int wkeys,
                                                       CompactIn ci, int B) {
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < count;
    const uint2 e = live ? list[idx] : make_uint2(0, 1u << 8);
    const uint64_t st = e.x;
    const uint32_t len = e.y >> 8;
    const uint64_t *sk = (e.y & 1) ? k1 : k0;
    const uint32_t *sv = (e.y & 1) ? v1 : v0;
    uint64_t key[kTiny];
    uint32_t val[kTiny];
    const uint64_t pf = live && ci.pref ? ci.pref[idx] : 0;
    const int ehi = (e.y >> 1) & 127;
#pragma unroll
    for (int j = 0; j < kTiny; ++j) {
        const uint64_t at = st + min((uint32_t)j, len - 1);
        const uint64_t x = live ? sk[at] : 0;
        key[j] = (pf & kCompact) ? compact_key(pf, ehi, B, ci.nd[at], (uint32_t)(x >> 32)) : x;
        val[j] = !live ? 0 : (pf & kCompact) ? (uint32_t)x : sv[at];
    }
    uint32_t out[kTiny];
    bool hd[kTiny];
#pragma unroll
    for (int j = 0; j < kTiny; ++j) {
        uint32_t lt = 0, eq = 0;
#pragma unroll
        for (int i = 0; i < kTiny; ++i) {
            lt += (uint32_t)i < len && key[i] < key[j];
            eq += i < j && key[i] == key[j];
        }
        out[j] = lt + eq;
        hd[j] = eq == 0;
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < kTiny; ++j) {
        if ((uint32_t)j >= len) break;
        v0[st + out[j]] = val[j];
        if (wkeys) k0[st + out[j]] = key[j];
        heads[st + out[j]] = hd[j] ? 1 : 0;
    }
}

}  // namespace gkm
