// gkm_rankcheck.hip -- the check of the LDS lane order that the partitions' ranking relies on, run by
// gk_create once per device and process, and gk_rank_mode.  (This code object's own g_rank_ballot is
// never set: the check kernel names rank_ballot<> where it wants it.)
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>

#include "gkm_internal.h"
#include "gkm_partition.h"

using namespace gkm;

// Every partition of the sort ranks an item by one returning LDS atomic (rank_atomic,
// gkm_partition.h): it relies on the LDS applying the same-address lanes of one wave instruction in
// increasing lane order.  That is how gfx950 behaves (tools/lds_rank_probe.hip: no exception in
// 4e10 lane-ranks), not an ISA guarantee, so it is checked once per device and process against a
// ballot-match ground truth over every digit space the partitions rank in -- 2048, 1024, 512, 256,
// 128, 64, 16, 4 and 1 digits (the wide L0's 11 bits, the wave kernels' 10 / 9 / 8, the level
// passes' 8, L0's 7) with per-wave counter arrays of 2048 words, in both counter forms (u32 words,
// and the u16 halves of rank_atomic16), 8 items per trial, lanes sitting out, every CU busy.  Where
// it does not hold, the partitions switch to ballot-match ranking (rank_ballot): the same ranks
// from ballots alone.  The kernel checks that path as well.
__global__ __launch_bounds__(256) void lds_rank_check_kernel(uint32_t trials, unsigned long long *bad) {
    __shared__ uint32_t s_cnt[4][2048];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *cnt = s_cnt[wave];
    unsigned long long nb = 0;
    for (uint32_t t = 0; t < trials; ++t) {
        constexpr uint32_t kMasks[9] = {2047u, 1023u, 511u, 255u, 127u, 63u, 15u, 3u, 0u};
        const uint32_t dmask = kMasks[t % 9];
        const uint32_t form = (t / 9) & 3;  // 0 atomic u32, 1 ballot u32, 2 atomic u16, 3 ballot u16
        const bool ballot = form & 1;
#pragma unroll
        for (int u = 0; u < 32; ++u) cnt[u * 64 + lane] = 0;
        uint32_t dd[8], got[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t x = (blockIdx.x * 0x9E3779B9u) ^ (t * 0x85EBCA6Bu) ^ ((uint32_t)(i * 64 + lane) * 0xC2B2AE35u);
            x ^= x >> 15;
            x *= 0x2C1B3C6Du;
            x ^= x >> 12;
            dd[i] = x & dmask;
            const bool valid = ((x >> 20) & 7u) != 0;  // some lanes sit out
            const uint32_t d = dd[i], sh = (d & 1u) << 4;
            if (form == 0) got[i] = valid ? atomicAdd(&cnt[d], 1u) : 0u;
            else if (form == 1) got[i] = rank_ballot<11, false>(cnt, d, valid);
            else if (form == 2) got[i] = valid ? (atomicAdd(&cnt[d >> 1], 1u << sh) >> sh) & 0xFFFFu : 0u;
            else got[i] = rank_ballot<11, true>(cnt, d, valid);
            if (!valid) got[i] = ~0u;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool valid = got[i] != ~0u;
            // ground truth: valid lanes with the same digit below this lane, and in earlier items
            uint32_t want = 0;
            for (int j = 0; j <= i; ++j) {
                uint64_t m = __ballot(got[j] != ~0u);
#pragma unroll
                for (int b = 0; b < 11; ++b) {
                    const uint64_t x = __ballot((dd[j] >> b) & 1u);
                    m &= ((dd[i] >> b) & 1u) ? x : ~x;
                }
                want += (uint32_t)__popcll(j < i ? m : (m & ((1ull << lane) - 1ull)));
            }
            nb += (valid && got[i] != want) ? (ballot ? (1ull << 40) : 1ull) : 0ull;
        }
    }
    if (nb) atomicAdd(bad, nb);
}

namespace {
struct RankState {
    int checked = 0;  // 0 unchecked, 1 lane order holds, -1 it does not
    int forced = 0;   // ballot-match forced by gk_rank_mode (tests)
    int active = 0;   // ranking in use: 0 atomic, 1 ballot-match
};
std::mutex g_rank_mu;
std::map<int, RankState> g_rank;  // per device (hipGetDeviceCount-sized by use)

bool env_force_ballot() {
    const char *v = opt("GKM_RANK_BALLOT");
    return v && *v && std::strcmp(v, "0") != 0;
}

hipError_t set_rank_mode_all(int ballot) {
    hipError_t e = gkm::rank_mode_msd(ballot);
    if (e == hipSuccess) e = gkm::rank_mode_sort(ballot);
    return e;
}
}  // namespace

// the check on the current device (once per process), then its ranking mode
int gkm::lds_rank_check(int device) {
    std::lock_guard<std::mutex> lock(g_rank_mu);
    RankState &st = g_rank[device];
    if (st.checked == 0) {
        unsigned long long *d = nullptr, h = 0;
        if (hipMalloc(&d, 8) != hipSuccess) return GK_E_HIP;
        hipError_t e = hipMemset(d, 0, 8);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(lds_rank_check_kernel, dim3(2048), dim3(256), 0, 0, 72u, d);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        hipFree(d);
        if (e != hipSuccess) return GK_E_HIP;
        if (h >> 40) {  // the ballot-match ranking itself is wrong: nothing on this device can sort
            std::fprintf(stderr, "libgkm: device %d: ballot-match ranks differ from their ground truth (%llu)\n",
                         device, h >> 40);
            return GK_E_UNSUPPORTED;
        }
        st.checked = h == 0 ? 1 : -1;
        if (h)
            std::fprintf(stderr, "libgkm: device %d: a returning LDS atomic did not apply same-address lanes in "
                                 "lane order (%llu of ~1.9e8 ranks differ); the partitions rank by ballots instead\n",
                         device, h);
    }
    const int want = (st.checked < 0 || st.forced || env_force_ballot()) ? 1 : 0;
    if (hipError_t e = set_rank_mode_all(want); e != hipSuccess) return GK_E_HIP;
    st.active = want;
    return GK_OK;
}

extern "C" int gk_rank_mode(gk_ctx *c, int mode, int *active) {
    if (!c || mode < -1 || mode > 1) return GK_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return GK_E_HIP;
    std::lock_guard<std::mutex> lock(g_rank_mu);
    RankState &st = g_rank[c->device];
    if (mode >= 0) {
        st.forced = mode == 1;
        const int want = (st.forced || st.checked < 0 || env_force_ballot()) ? 1 : 0;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return GK_E_HIP;  // no launch of the old mode in flight
        if (set_rank_mode_all(want) != hipSuccess) return GK_E_HIP;
        st.active = want;
    }
    if (active) *active = st.active;
    return GK_OK;
}
