// gkm_lcp.hip -- gk_lcp: the longest common prefix of every sorted k-mer with its predecessor, cached
// as a view of the sorted order, and what is read off it (gfx950): the k-mer spectrum for every length
// at once (gk_lcp_spectrum) and the per-position tracks (gk_position_track).
//
// lcp[q] (q >= 1) = the largest k in 0..cap at which sorted k-mers q - 1 and q compare equal under
// sba_equal (gkm_group.hip; kmers.py:306-397) at kmer_len = k; lcp[0] = 0, and lcp[n] = 0 wherever a
// successor is read.  The group head at any k in 1..cap is lcp[q] < k.  Two paths, the same answers
// (gkm_lcp_host.h; DESIGN.md §4, "LCP, spectrum and position tracks"):
//   keys   the encoded keys decide prefixes (the conditions under which group_front compares masked
//          keys at every length: direct keys without a length field): XOR with the predecessor's key,
//          count leading zeros, divide by the bits per symbol.  8 W bytes read and 4 written per k-mer;
//          the predecessor's key comes from the lane below, lane 0 of each wave loads it.
//   bytes  everything else on a forward order: sba_equal's loop over the two windows, counting.
// The spectrum is one pass over the array: the histograms of lcp[q] and of max(lcp[q], lcp[q + 1]),
// reduced in the wave, then in the block's LDS, then by one global atomic per block and bin; their
// prefix sums (host, cap + 1 values) are distinct[k] and unique[k].  The tracks scatter one
// 4-byte value per k-mer to its start position in a zero-filled uint32[sba_len].
#include <algorithm>
#include <vector>

#include "gkm_internal.h"
#include "gkm_lcp_host.h"
#include "gkm_query_host.h"

namespace gkm {

constexpr int kLcpMaxBlocks = 2048;  // 8 blocks per CU; the rest by grid stride

// ---------------------------------------------------------------------------------------------
// the array
// ---------------------------------------------------------------------------------------------
// Position tile0 + j * kThreads + thread, j < kItems: every load of a tile is issued before the first
// comparison.  All lanes run the shuffles (a lane past n holds zeros and stores nothing).
template <int W>
__global__ __launch_bounds__(lcp::kThreads) void lcp_keys_kernel(const uint64_t *__restrict__ keys, uint64_t n, int bits,
                                                                 int symbols, uint32_t cap,
                                                                 uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tiles = (n + lcp::kTile - 1) / lcp::kTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t tile0 = t * lcp::kTile;
        uint64_t k[lcp::kItems][W], halo[lcp::kItems][W];
#pragma unroll
        for (uint32_t j = 0; j < lcp::kItems; ++j) {
            const uint64_t i = tile0 + j * lcp::kThreads + threadIdx.x;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                k[j][w] = i < n ? keys[(uint64_t)w * n + i] : 0;
                halo[j][w] = (lane == 0 && i > 0 && i < n) ? keys[(uint64_t)w * n + i - 1] : 0;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < lcp::kItems; ++j) {
            const uint64_t i = tile0 + j * lcp::kThreads + threadIdx.x;
            uint64_t p[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t below = (uint64_t)__shfl_up((unsigned long long)k[j][w], 1);
                p[w] = lane == 0 ? halo[j][w] : below;
            }
            if (i < n) out[i] = i == 0 ? 0u : lcp::keys_lcp<W>(p, k[j], bits, symbols, cap);
        }
    }
}

__global__ __launch_bounds__(lcp::kThreads) void lcp_bytes_kernel(const uint8_t *__restrict__ sba,
                                                                  const uint32_t *__restrict__ starts, uint64_t n,
                                                                  uint32_t cap, uint32_t *__restrict__ out) {
    for (uint64_t q = blockIdx.x * (uint64_t)lcp::kThreads + threadIdx.x; q < n; q += (uint64_t)gridDim.x * lcp::kThreads)
        out[q] = q == 0 ? 0u : lcp::bytes_lcp(sba, starts[q - 1], starts[q], cap);
}

// ---------------------------------------------------------------------------------------------
// pairs (lcp[q], lcp[q + 1]): the spectrum and the min_unique track
// ---------------------------------------------------------------------------------------------
// For this thread's kItems positions of the tile at tile0: a = min(lcp[q], cap) and m = max(a,
// min(lcp[q + 1], cap)), lcp[n] = 0.  lcp[q + 1] comes from the lane above; lane 63 loads it.
__device__ __forceinline__ void load_pairs(const uint32_t *__restrict__ lcpv, uint64_t n, uint64_t tile0, uint32_t cap,
                                           uint32_t (&a)[lcp::kItems], uint32_t (&m)[lcp::kItems]) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t halo[lcp::kItems];
#pragma unroll
    for (uint32_t j = 0; j < lcp::kItems; ++j) {
        const uint64_t i = tile0 + j * lcp::kThreads + threadIdx.x;
        a[j] = i < n ? min(lcpv[i], cap) : 0u;
        halo[j] = (lane == 63 && i + 1 < n) ? min(lcpv[i + 1], cap) : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < lcp::kItems; ++j) {
        const uint32_t above = __shfl_down(a[j], 1);
        m[j] = max(a[j], lane == 63 ? halo[j] : above);
    }
}

// One count into bin `bin` of every lane with `active`, reduced within the wave first: in each round
// the lanes that hold the first active lane's bin are counted by one ballot and added by that lane
// alone; the lanes left after kPeelRounds rounds add one each.  A random genome puts almost every
// value on three or four bins near log4(n) and a repeat puts half a wave or all of it on cap: the
// first round takes the largest share off the LDS atomics' same-address queue, and every further
// round cost more than it saved (gkm_lcp_host.h, profiles/lcp/ab_peel.txt).  Bins below lds_bins
// are the block's (LDS), the others global.  Called by every lane of the wave.
__device__ __forceinline__ void wave_hist_add(uint32_t *s_bins, unsigned long long *__restrict__ g_bins, uint32_t bin,
                                              bool active, uint32_t lds_bins) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < lcp::kPeelRounds; ++r) {
        const unsigned long long live = __ballot(active);
        if (live == 0) break;  // wave-uniform
        const uint32_t first = (uint32_t)__ffsll((long long)live) - 1;
        const uint32_t b0 = __shfl(bin, (int)first);
        const bool mine = active && bin == b0;
        const unsigned long long same = __ballot(mine);
        if (lane == first) {
            const uint32_t cnt = (uint32_t)__popcll(same);
            if (b0 < lds_bins) atomicAdd(&s_bins[b0], cnt);
            else atomicAdd(&g_bins[b0], (unsigned long long)cnt);
        }
        if (mine) active = false;
    }
    if (active) {
        if (bin < lds_bins) atomicAdd(&s_bins[bin], 1u);
        else atomicAdd(&g_bins[bin], 1ull);
    }
}

// hist[0][v] += #{q : min(lcp[q], cap) == v}, hist[1][v] += #{q : max(lcp[q], lcp[q + 1]) clamped == v};
// hist: two rows of cap + 1 bins.  A block counts fewer than 2^32 positions, so its LDS bins do not
// wrap.  The block's bins leave it by one global atomic per bin that is not 0: writing them as rows
// for a second kernel to add up instead was measured 0.03 ms slower at 1e8 k-mers, the second launch
// costing more than 2,048 blocks' atomics on the same few lines (profiles/lcp/ab_flush_peel.txt).
__global__ __launch_bounds__(lcp::kThreads) void lcp_spectrum_kernel(const uint32_t *__restrict__ lcpv, uint64_t n,
                                                                     uint32_t cap,
                                                                     unsigned long long *__restrict__ hist) {
    __shared__ uint32_t s_bins[2][lcp::kLdsBins];
    const uint32_t lds_bins = cap + 1 < lcp::kLdsBins ? cap + 1 : lcp::kLdsBins;
    for (uint32_t b = threadIdx.x; b < lds_bins; b += lcp::kThreads) s_bins[0][b] = s_bins[1][b] = 0;
    __syncthreads();
    unsigned long long *hist_m = hist + (uint64_t)cap + 1;
    const uint64_t tiles = (n + lcp::kTile - 1) / lcp::kTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t tile0 = t * lcp::kTile;
        uint32_t a[lcp::kItems], m[lcp::kItems];
        load_pairs(lcpv, n, tile0, cap, a, m);
#pragma unroll
        for (uint32_t j = 0; j < lcp::kItems; ++j) {
            const bool valid = tile0 + j * lcp::kThreads + threadIdx.x < n;
            wave_hist_add(s_bins[0], hist, a[j], valid, lds_bins);
            wave_hist_add(s_bins[1], hist_m, m[j], valid, lds_bins);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < lds_bins; b += lcp::kThreads) {
        if (s_bins[0][b]) atomicAdd(&hist[b], (unsigned long long)s_bins[0][b]);
        if (s_bins[1][b]) atomicAdd(&hist_m[b], (unsigned long long)s_bins[1][b]);
    }
}

// track[starts[q]] = the shortest unique length of sorted k-mer q (track zero-filled; starts < sba_len)
__global__ __launch_bounds__(lcp::kThreads) void track_min_unique_kernel(const uint32_t *__restrict__ lcpv,
                                                                         const uint32_t *__restrict__ starts,
                                                                         uint64_t n, uint32_t cap,
                                                                         uint32_t *__restrict__ track) {
    const uint64_t tiles = (n + lcp::kTile - 1) / lcp::kTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t tile0 = t * lcp::kTile;
        uint32_t a[lcp::kItems], m[lcp::kItems], s[lcp::kItems];
#pragma unroll
        for (uint32_t j = 0; j < lcp::kItems; ++j) {
            const uint64_t i = tile0 + j * lcp::kThreads + threadIdx.x;
            s[j] = i < n ? starts[i] : 0u;
        }
        load_pairs(lcpv, n, tile0, cap, a, m);
#pragma unroll
        for (uint32_t j = 0; j < lcp::kItems; ++j)
            if (tile0 + j * lcp::kThreads + threadIdx.x < n) track[s[j]] = lcp::min_unique_of(m[j], cap);
    }
}

// track[starts[q]] = the size of q's group: gid[q] = the inclusive scan of the head flags (q's group
// is gid[q] - 1; the first flag is set), gstart = the G group starts
__global__ __launch_bounds__(lcp::kThreads) void track_multiplicity_kernel(const uint32_t *__restrict__ gid,
                                                                           const uint32_t *__restrict__ gstart,
                                                                           uint64_t G,
                                                                           const uint32_t *__restrict__ starts,
                                                                           uint64_t n, uint32_t *__restrict__ track) {
    for (uint64_t q = blockIdx.x * (uint64_t)lcp::kThreads + threadIdx.x; q < n; q += (uint64_t)gridDim.x * lcp::kThreads) {
        const uint64_t next = gid[q];
        const uint64_t g = next ? next - 1 : 0;
        const uint64_t end = next < G ? (uint64_t)gstart[next] : n;
        track[starts[q]] = (uint32_t)(end - gstart[g]);
    }
}

// ---------------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------------
static unsigned lcp_grid(uint64_t n) {
    const uint64_t tiles = (n + lcp::kTile - 1) / lcp::kTile;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kLcpMaxBlocks);
}

// the preconditions every call shares: a sequence and a sorted k-mer set
static int lcp_state_checks(gk_ctx *c, const char *what) {
    if (!c->sba) return fail(c, GK_E_STATE, std::string(what) + ": no sequence loaded");
    if (!c->have_starts || !c->sorted)
        return fail(c, GK_E_STATE, std::string(what) + ": the k-mers are not sorted: call gk_sort first");
    return GK_OK;
}

// ... and of the calls that need prefixes: a cap in range, a forward order
static int lcp_prefix_checks(gk_ctx *c, const char *what, uint32_t max_len) {
    if (int rc = lcp_state_checks(c, what)) return rc;
    if (max_len == 0) return fail(c, GK_E_ARG, std::string(what) + ": max_len must be >= 1");
    if (max_len > lcp::kMaxCap)
        return fail(c, GK_E_ARG, std::string(what) + ": max_len (" + std::to_string(max_len) + ") is above 2^24");
    if (c->sort_len != 0 && max_len > c->sort_len)
        return fail(c, GK_E_ARG, std::string(what) + ": max_len (" + std::to_string(max_len) +
                                     ") is above the sort length (" + std::to_string(c->sort_len) + ")");
    if (c->canonical)
        return fail(c, GK_E_UNSUPPORTED,
                    std::string("canonical k-mers have no prefixes: ") + what + " needs a forward order");
    return GK_OK;
}

// the view at a cap >= `cap`, built unless the cached one serves (a reader clamps to its own cap)
static int lcp_ensure(gk_ctx *c, uint32_t cap, uint32_t **out) {
    const KeySpec &ks = c->spec;
    const bool keys_ok = c->keys_valid && !c->keys_are_ranks && ks.lenbits == 0 && (ks.bits == 2 || ks.bits == 4) &&
                         ks.words >= 1 && ks.words <= kMaxWords && ks.symbols >= 1;
    const int path = query::parse_path(opt("GKM_LCP_PATH"));
    if (path < 0) return fail(c, GK_E_ARG, "GKM_LCP_PATH must be 'bytes' or 'keys'");
    if (path == query::kPathKeys && !keys_ok)
        return fail(c, GK_E_UNSUPPORTED, "GKM_LCP_PATH=keys: the context holds no direct keys without a length field");
    const bool use_keys = keys_ok && path != query::kPathBytes;
    GK_TRY_HIP(c, hipSetDevice(c->device));
    const uint64_t n = c->n;
    GK_TRY_HIP(c, scratch(c, "lcp", n, out));
    if (c->lcp_valid && c->lcp_cap >= cap && c->lcp_bytes == !use_keys) return GK_OK;
    c->lcp_valid = false;
    if (int rc = materialize_starts(c)) return rc;
    if (n > 0 && use_keys) {
        if (int rc = ensure_keys(c)) return rc;
        const uint64_t *keys = c->keys[c->cur];
        const dim3 grid(lcp_grid(n)), block(lcp::kThreads);
        int slot;
        timer_begin(c, "lcp_keys", &slot);
        timer_units(c, slot, n);
        switch (ks.words) {
        case 1: hipLaunchKernelGGL((lcp_keys_kernel<1>), grid, block, 0, c->stream, keys, n, ks.bits, ks.symbols, cap, *out); break;
        case 2: hipLaunchKernelGGL((lcp_keys_kernel<2>), grid, block, 0, c->stream, keys, n, ks.bits, ks.symbols, cap, *out); break;
        case 3: hipLaunchKernelGGL((lcp_keys_kernel<3>), grid, block, 0, c->stream, keys, n, ks.bits, ks.symbols, cap, *out); break;
        default: hipLaunchKernelGGL((lcp_keys_kernel<4>), grid, block, 0, c->stream, keys, n, ks.bits, ks.symbols, cap, *out); break;
        }
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
    } else if (n > 0) {
        int slot;
        timer_begin(c, "lcp_bytes", &slot);
        timer_units(c, slot, n);
        hipLaunchKernelGGL(lcp_bytes_kernel, dim3(grid_of(n, kLcpMaxBlocks)), dim3(lcp::kThreads), 0, c->stream, c->sba,
                           c->vals[c->cur], n, cap, *out);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
    }
    c->lcp_valid = true;
    c->lcp_bytes = !use_keys;
    c->lcp_cap = c->lcp_asked = cap;
    return GK_OK;
}

// the zero-filled track of the current sequence (scratch "track")
static int track_reset(gk_ctx *c, uint32_t **out) {
    c->track_len = 0;
    GK_TRY_HIP(c, scratch(c, "track", c->sba_len, out));
    if (c->sba_len) GK_TRY_HIP(c, hipMemsetAsync(*out, 0, 4 * c->sba_len, c->stream));
    return GK_OK;
}

}  // namespace gkm

using namespace gkm;

extern "C" int gk_lcp(gk_ctx *c, uint32_t max_len, uint64_t *n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (int rc = lcp_prefix_checks(c, "gk_lcp", max_len)) return rc;
    uint32_t *d_lcp;
    if (int rc = lcp_ensure(c, max_len, &d_lcp)) return rc;
    c->lcp_asked = max_len;
    if (n) *n = c->n;
    return GK_OK;
}

extern "C" int gk_copy_lcp(gk_ctx *c, uint64_t offset, uint32_t *dst, uint64_t count) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->lcp_valid) return fail(c, GK_E_STATE, "call gk_lcp first");
    if (offset > c->n || count > c->n - offset) return fail(c, GK_E_ARG, "range outside the k-mer array");
    if (count == 0) return GK_OK;
    if (!dst) return fail(c, GK_E_ARG, "null array");
    uint32_t *d_lcp;
    GK_TRY_HIP(c, scratch(c, "lcp", c->n, &d_lcp));
    GK_TRY_HIP(c, hipMemcpyAsync(dst, d_lcp + offset, 4 * count, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (c->lcp_asked < c->lcp_cap)  // a view built for a larger cap serves this one
        for (uint64_t i = 0; i < count; ++i) dst[i] = std::min(dst[i], c->lcp_asked);
    return GK_OK;
}

extern "C" int gk_device_lcp(gk_ctx *c, void **lcp_out, uint64_t *n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->lcp_valid) return fail(c, GK_E_STATE, "call gk_lcp first");
    uint32_t *d_lcp;
    GK_TRY_HIP(c, scratch(c, "lcp", c->n, &d_lcp));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (lcp_out) *lcp_out = d_lcp;
    if (n) *n = c->n;
    return GK_OK;
}

extern "C" int gk_lcp_spectrum(gk_ctx *c, uint32_t max_len, uint64_t *distinct, uint64_t *unique) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (int rc = lcp_prefix_checks(c, "gk_lcp_spectrum", max_len)) return rc;
    if (!distinct || !unique) return fail(c, GK_E_ARG, "gk_lcp_spectrum: null array");
    uint32_t *d_lcp;
    if (int rc = lcp_ensure(c, max_len, &d_lcp)) return rc;
    const uint64_t bins = (uint64_t)max_len + 1;
    unsigned long long *d_hist;
    GK_TRY_HIP(c, scratch(c, "lcp_hist", 2 * bins, &d_hist));
    GK_TRY_HIP(c, hipMemsetAsync(d_hist, 0, 16 * bins, c->stream));
    if (c->n > 0) {
        int slot;
        timer_begin(c, "lcp_spectrum", &slot);
        timer_units(c, slot, c->n);
        hipLaunchKernelGGL(lcp_spectrum_kernel, dim3(lcp_grid(c->n)), dim3(lcp::kThreads), 0, c->stream, d_lcp, c->n,
                           max_len, d_hist);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
    }
    std::vector<unsigned long long> h(2 * bins);
    GK_TRY_HIP(c, hipMemcpyAsync(h.data(), d_hist, 16 * bins, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    // distinct[k] = #{lcp < k}, unique[k] = #{max(lcp[q], lcp[q + 1]) < k}; entry 0 is unused
    uint64_t sd = 0, su = 0;
    for (uint64_t k = 0; k < bins; ++k) {
        distinct[k] = sd;
        unique[k] = su;
        sd += h[k];
        su += h[bins + k];
    }
    return GK_OK;
}

extern "C" int gk_position_track(gk_ctx *c, int kind, uint32_t len, uint32_t *dst, uint64_t sba_len) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (kind != GK_TRACK_MIN_UNIQUE && kind != GK_TRACK_MULTIPLICITY)
        return fail(c, GK_E_ARG, "gk_position_track: kind (" + std::to_string(kind) +
                                     ") must be GK_TRACK_MIN_UNIQUE (1) or GK_TRACK_MULTIPLICITY (2)");
    uint32_t *track = nullptr;
    const uint64_t n = c->n;
    if (kind == GK_TRACK_MIN_UNIQUE) {
        if (int rc = lcp_prefix_checks(c, "gk_position_track", len)) return rc;
    } else {
        if (int rc = lcp_state_checks(c, "gk_position_track")) return rc;
        if (c->sort_len != 0 && len > c->sort_len)
            return fail(c, GK_E_ARG, "gk_position_track: kmer_len (" + std::to_string(len) +
                                         ") is above the sort length (" + std::to_string(c->sort_len) + ")");
    }
    if (sba_len != c->sba_len)
        return fail(c, GK_E_ARG, "gk_position_track: sba_len (" + std::to_string(sba_len) +
                                     ") differs from the sequence's length (" + std::to_string(c->sba_len) + ")");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (kind == GK_TRACK_MIN_UNIQUE) {
        uint32_t *d_lcp;
        if (int rc = lcp_ensure(c, len, &d_lcp)) return rc;
        if (int rc = track_reset(c, &track)) return rc;
        if (n > 0) {
            int slot;
            timer_begin(c, "track_min_unique", &slot);
            timer_units(c, slot, n);
            hipLaunchKernelGGL(track_min_unique_kernel, dim3(lcp_grid(n)), dim3(lcp::kThreads), 0, c->stream, d_lcp,
                               c->vals[c->cur], n, len, track);
            GK_TRY_HIP(c, hipGetLastError());
            timer_end(c, slot);
        }
    } else {
        // the groups at kmer_len (0: the sort length; None on a suffix order), every k-mer kept
        const uint32_t kl = len ? len : c->sort_len;
        uint64_t G = 0;
        const uint8_t *heads = nullptr;
        if (int rc = group_starts_all(c, kl ? (int64_t)kl : -1, &G, &heads)) return rc;
        if (int rc = track_reset(c, &track)) return rc;
        if (n > 0) {
            if (!heads || G == 0) return fail(c, GK_E_STATE, "gk_position_track: the group pass left no head flags");
            GK_TRY_HIP(c, scan_flags_inclusive(c, heads, n, c->idx_a));
            int slot;
            timer_begin(c, "track_multiplicity", &slot);
            timer_units(c, slot, n);
            hipLaunchKernelGGL(track_multiplicity_kernel, dim3(grid_of(n, kLcpMaxBlocks)), dim3(lcp::kThreads), 0,
                               c->stream, c->idx_a, c->idx_b, G, c->vals[c->cur], n, track);
            GK_TRY_HIP(c, hipGetLastError());
            timer_end(c, slot);
        }
    }
    if (dst && sba_len) GK_TRY_HIP(c, hipMemcpyAsync(dst, track, 4 * sba_len, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    c->track_len = sba_len;
    return GK_OK;
}

extern "C" int gk_device_track(gk_ctx *c, void **track_out, uint64_t *sba_len) {
    if (!c) return GK_E_ARG;
    if (c->track_len == 0) return fail(c, GK_E_STATE, "call gk_position_track first");
    uint32_t *track;
    GK_TRY_HIP(c, scratch(c, "track", c->track_len, &track));
    if (track_out) *track_out = track;
    if (sba_len) *sba_len = c->track_len;
    return GK_OK;
}
