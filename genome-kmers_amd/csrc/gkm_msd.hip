// gkm_msd.hip -- MSD radix sort of one-word k-mer keys (the C3 hot path), gfx950.
//
// An LSD sort of 62-bit keys moves every (key, start) pair 8 times.  Here each pass partitions
// only what is still unsorted, and buckets small enough for LDS are finished there:
//   L0     encode + partition by the top 8 bits, straight from the sequence byte array
//   L1..   partition every bucket larger than kBlockMax by the next 8 bits
//   local  buckets of kWaveMax+1..kBlockMax elements: one 256-thread workgroup each; buckets of
//          1..kWaveMax: one wave each.  The bucket is partitioned by its next digit in LDS,
//          sub-buckets of <= kSmall are finished by rank-by-count, and the bucket is written
//          back once, with its group-head flags; larger sub-buckets go to another round.
// For 3.1e9 random 31-mers: L0, L1, L2 and one wave-local round -- 4 movements of the data.
//
// Order contract: equal keys come out by ascending start index, the reference's break_ties=True
// order (kmers.py:1710-1711).  Every partition here is STABLE (64-lane ballot-match ranking,
// tiles and workgroups in input order) and the L0 input is in ascending start order, so equal
// keys stay in start order without ever comparing starts; a sub-bucket whose key bits are
// exhausted is final as it stands.  Every global partition offset is known before its scatter
// starts (count pass + column scan of per-tile digit histograms): no look-back chain.
//
// This file is the host side: the driver (MsdDriver) and the entry points.  The kernels are in the
// stage headers included below (gkm_msd_l0.h, _scan.h, _lists.h, _local.h, _ties.h), their constants
// in gkm_msd_config.h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gkm_canon.h"
#include "gkm_internal.h"
#include "gkm_msd_config.h"
#include "gkm_partition.h"
#include "gkm_swar.h"

namespace gkm {

__constant__ uint8_t c_code4_msd[256];
static bool g_msd_tables = false;

static hipError_t msd_tables() {
    if (g_msd_tables) return hipSuccess;
    uint8_t code4[256] = {0};
    const char *order = "ABCDGHKMNRSTVWY";
    for (int i = 0; order[i]; ++i) code4[(uint8_t)order[i]] = (uint8_t)(i + 1);
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_code4_msd), code4, 256);
    if (e == hipSuccess) g_msd_tables = true;
    return e;
}

}  // namespace gkm

// the device code, by stage (private to this file; after c_code4_msd, which the kernels read)
#include "gkm_msd_l0.h"
#include "gkm_msd_scan.h"
#include "gkm_msd_lists.h"
#include "gkm_msd_local.h"
#include "gkm_msd_ties.h"

namespace gkm {

// ---------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------
// blocks of 256 threads over n items, two clamps: at least one block, as many as n needs (lists of
// buckets, one thread each: an empty list still launches); or at most 65,536 blocks, none for
// n = 0 (grid-stride kernels over elements)
static int grid256_min1(uint64_t n) { return (int)std::max<uint64_t>((n + 255) / 256, 1); }
static unsigned grid256_cap64k(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 16); }

// grow a device array to hold `need` entries, keeping the first `keep` entries
template <typename T>
static hipError_t grow_keep(gk_ctx *c, const char *name, uint64_t need, uint64_t keep, T **p) {
    auto &e = c->scratch[name];
    if (e.first && e.second >= sizeof(T) * need) {
        *p = static_cast<T *>(e.first);
        return hipSuccess;
    }
    void *np = nullptr;
    const uint64_t bytes = sizeof(T) * (need + need / 2 + 256);
    hipError_t r = dev_alloc(&np, bytes);
    if (r != hipSuccess) return r;
    if (e.first && keep) {
        r = hipMemcpyAsync(np, e.first, sizeof(T) * keep, hipMemcpyDeviceToDevice, c->stream);
        if (r != hipSuccess) return r;
        r = hipStreamSynchronize(c->stream);
        if (r != hipSuccess) return r;
    }
    if (e.first) dev_free(e.first);
    e.first = np;
    e.second = bytes;
    *p = static_cast<T *>(np);
    return hipSuccess;
}

static unsigned cu_count(gk_ctx *c) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 8) cus = 256;
    return (unsigned)(cus / 8 * 8);
}

// resident workgroups per CU (>= 1) of kernel `fn` at `threads` per workgroup: what sizes a
// persistent grid.  Asked of the runtime once per context, kernel and block size, so no launch pays
// for the query again; a query that fails answers 1 and is asked again next time
static unsigned resident_per_cu(gk_ctx *c, const void *fn, int threads) {
    auto it = c->occupancy.find({fn, threads});
    if (it != c->occupancy.end()) return (unsigned)it->second;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0) != hipSuccess || per_cu < 1)
        return 1;  // (not cached: the next launch asks again)
    c->occupancy[{fn, threads}] = per_cu;
    return (unsigned)per_cu;
}


// tuning only (A/B runs): GKM_NO_COMPACT=1 keeps 64-bit keys in every level's output
static bool no_compact() { return opt("GKM_NO_COMPACT") != nullptr; }  // (read per level: tests flip it)

// (the transfer's resident copy: stops at every non-ACGT byte, pack2_word<true>)
hipError_t launch_pack2(const uint8_t *from, uint64_t nwords, uint64_t *code, uint32_t *dol, hipStream_t s) {
    if (nwords == 0) return hipSuccess;
    hipLaunchKernelGGL(pack2_kernel<true>, dim3((unsigned)std::min<uint64_t>((nwords + 255) / 256, 65536)), dim3(256),
                       0, s, from, nwords, code, dol);
    return hipGetLastError();
}

// the packed copy of c->sba (pack2_kernel) over the whole padded array, for ACGT sequences: only
// where the transfer left no resident packed copy and the pass needs one (the starts-only shard
// sort).  Packing before every sort did not pay: the L0 partition got slower reading packed words
// (17.8 vs 16.4 ms at C3) and the key-range passes gained less than the 0.8 ms the packing costs
static int pack_sequence(gk_ctx *c, const uint64_t **code, const uint32_t **dol) {
    const uint64_t nwords = (c->sba_len + kSbaPad) / 32;  // sba_cap >= sba_len + kSbaPad
    uint64_t *pc;
    uint32_t *pd;
    GK_TRY_HIP(c, scratch(c, "pk_code", nwords, &pc));
    GK_TRY_HIP(c, scratch(c, "pk_dol", nwords, &pd));
    int slot;
    timer_begin(c, "msd_pack", &slot);
    timer_units(c, slot, c->sba_len);
    hipLaunchKernelGGL(pack2_kernel<false>, dim3((unsigned)std::min<uint64_t>((nwords + 255) / 256, 65536)), dim3(256),
                       0, c->stream, c->sba, nwords, pc, pd);
    GK_TRY_HIP(c, hipGetLastError());
    timer_end(c, slot);
    *code = pc;
    *dol = pd;
    return GK_OK;
}

static const char *kLocPrefName[kLocal] = {"locp0", "locp1", "locp2", "locp3", "locp4", "locp5"};
static const char *kLocName[kLocal][2] = {{"loc0a", "loc0b"}, {"loc1a", "loc1b"}, {"loc2a", "loc2b"},
                                          {"loc3a", "loc3b"}, {"loc4a", "loc4b"}, {"loc5a", "loc5b"}};
static const char *kLocTimer[kLocal][2] = {{"msd_local_wave4", "msd_local_wave4_r"},
                                           {"msd_local_wave8", "msd_local_wave8_r"},
                                           {"msd_local_wave16", "msd_local_wave16_r"},
                                           {"msd_local_block16", "msd_local_block16_r"},
                                           {"msd_local_tiny", "msd_local_tiny_r"},
                                           {"msd_local_block32", "msd_local_block32_r"}};
static const char *kPassNames[] = {"msd_pass_l0", "msd_pass_l1", "msd_pass_l2", "msd_pass_l3",
                                   "msd_pass_l4", "msd_pass_l5", "msd_pass_l6", "msd_pass_l7"};
static const char *kPassNamesP[] = {"msd_pass_l0p", "msd_pass_l1p", "msd_pass_l2p", "msd_pass_l3p",
                                    "msd_pass_l4p", "msd_pass_l5p", "msd_pass_l6p", "msd_pass_l7p"};  // packed pairs
static const char *kPassNamesC[] = {"msd_pass_l0c", "msd_pass_l1c", "msd_pass_l2c", "msd_pass_l3c",
                                    "msd_pass_l4c", "msd_pass_l5c", "msd_pass_l6c", "msd_pass_l7c"};  // compact

// One MSD sort of one-word keys into keys[0] / vals[0] (+ group heads).  The first partition
// comes from the sequence (l0_count, l0_start) or from received buckets (first_level_from_pieces);
// the rest -- global levels while buckets exceed kBlockMax, local rounds, done copies, later phases
// (run_from) -- is common.  An entry point sets up with begin().
struct MsdDriver {
    gk_ctx *c;
    KeySpec ks;
    int B;
    uint64_t n = 0;
    unsigned cus, pgrid;
    int slot = -1, total_slot = -1;
    uint32_t *ctr = nullptr, h[kCtrN] = {0};
    unsigned long long *sums = nullptr, hs[kSumN] = {0};  // (one device block: ctr, then sums at byte 64)
    uint32_t *big_start[2], *big_len[2];
    uint64_t *big_pref[2];         // prefixes of the big-list buckets (Lists::nb_pref)
    uint64_t *loc_pref[kLocal];    // prefixes of generation 0's local entries (Lists::loc_pref)
    uint32_t *dn_start, *dn_len;
    uint8_t *dn_par;
    uint2 *loc[kLocal][2];
    int wsched[kMaxLevels];  // digit bits of global level l (L0: 7..8 for 2-bit keys, else 8; l >= 1: 6..8)
    int width(int level) const { return wsched[std::min(level, kMaxLevels - 1)]; }
    uint8_t *heads = nullptr;
    uint8_t *nd = nullptr;  // next-level digit per element of the last pass's output
    // The element format of the current buffer, i.e. of what the next level (or the classify behind
    // the last one) reads; a level's output format is chosen by level_format, what reads what by reads():
    //   KeyStart       64-bit keys and starts; the next level counts its digits from the keys
    //   KeyStartDigit  the same plus the next level's digit byte per element in nd
    //   Pairs          packed pairs (MODE 5): 10-byte (key bits below the sorted ones, start) + the
    //                  digit byte instead of 12-byte (key, start) + digit, written by the level before
    //                  a compact one, which reads them (IN79)
    //   Compact        (low key bits, start) + the next digit instead of keys and starts (see
    //                  classify_kernel): the local kernels rebuild the keys; the rare large
    //                  sub-buckets get theirs back at once (expand_big), so a next level reads them as
    //                  KeyStartDigit
    //   PackedL0       the packed L0's output (P88, msd0_pipe_kernel): (digit byte, packed pair) in
    //                  nd_l0 / lo16_l0 / keys
    enum class Fmt { KeyStart, KeyStartDigit, Pairs, Compact, PackedL0 };
    Fmt cur_fmt = Fmt::KeyStart;
    int compact_hi = 0;
    bool allow_c79 = false;  // packed-pair levels allowed (begin)
    bool p88 = false;        // the L0 writes PackedL0 (p88_wanted: l0_start's decision)
    int p88_shi = 0;
    uint16_t *lo16_l0 = nullptr;
    uint8_t *nd_l0 = nullptr;
    int c79_shi = 0;
    uint16_t *lo16 = nullptr;
    uint32_t *tile_hist, *chunk_hist, *c_first, *c_ntiles, *seg_base, *seg_cnt;
    uint64_t nloc[kLocal] = {0}, loc_elems[kLocal] = {0}, ndone = 0, big_elems = 0;
    uint32_t nbig = 0;
    int cur_big = 0;
    int phase = 0;  // key word being sorted (multi-word keys)
    uint32_t ctiles = kChunkTiles;  // tiles per column-scan chunk
    // final keys: the finishing kernels also write every key to keys[0], so a one-word sort ends
    // with sorted keys + starts + heads in HBM (no re-encode by gather afterwards)
    int wkeys = 0;
    bool acgt_keys = false;  // the caller of an acgt_only sort wants its final keys too (split_sort)
    // the L0 passes' arguments (l0_count fills them in; pk_code / pk_dol, the packed sequence, are set
    // beforehand by use_resident_pack) and tiles; key-range shards: the ownership digit range
    // [own_lo, own_lo + own_span) is kept
    L0Args l0a{};
    uint64_t l0_tiles = 0;

    MsdDriver(gk_ctx *c_, const KeySpec &ks_) : c(c_), ks(ks_), B(ks_.total_bits) {
        cus = cu_count(c);
        pgrid = cus * 4;  // 4 workgroups per CU, one resident at a time (LDS); measured faster than 1
        set_widths(opt("GKM_LEVEL_BITS"));
        // test-only: small scan chunks so that parity tests reach the multi-chunk branches of the
        // column scan and tile tables (otherwise only buckets > 2.9 M keys have more than one chunk)
        if (const char *e = opt("GKM_TEST_CHUNK_TILES")) ctiles = (uint32_t)std::max(1, std::atoi(e));
    }

    // the whole sort of forward 2-bit one-word keys (msd_sort's phase 0): an 11-bit L0
    // (msd0_wide_kernel) when GKM_WIDE_L0=1 (A/B), so that 11 + 8 bits leave C3-sized buckets for
    // one block-local round
    void enable_wide_l0() {
        const char *e = opt("GKM_WIDE_L0");  // (read per sort: tests flip it)
        const bool want = e && *e && std::strcmp(e, "0") != 0;
        if (want && ks.bits == 2 && !ks.canonical && !ks.acgt_only && B > kWideL0 + 8) wsched[0] = kWideL0;
    }

    // level digit widths "w0,w1,w2,..." (the last one repeats).  Default 7,8,8,...: for 2-bit
    // keys a 7-bit L0 is ~10% faster than an 8-bit one (longer runs per tile), and after 23 bits
    // the C3 buckets (~370) fit the one-wave finishing kernel; 4-bit keys keep an 8-bit L0.
    void set_widths(const char *spec) {
        for (int l = 0; l < kMaxLevels; ++l) wsched[l] = kGR;
        if (ks.bits == 2) wsched[0] = 7;
        if (!spec) return;
        int l = 0, w = kGR;
        for (const char *p = spec; *p && l < kMaxLevels;) {
            w = std::min(8, std::max(6, std::atoi(p)));
            wsched[l++] = w;
            while (*p && *p != ',') ++p;
            if (*p == ',') ++p;
        }
        for (; l < kMaxLevels; ++l) wsched[l] = w;
        if (ks.bits != 2) wsched[0] = kGR;
        wsched[0] = std::max(wsched[0], ks.canonical ? 7 : 6);  // (6: forward 2-bit L0 only)
    }

    Lists lists(int g, int bigsel) {
        // prefixes are recorded by classify (generation 0); re-listed entries carry full keys
        return Lists{big_start[bigsel], big_len[bigsel], dn_start, dn_len, dn_par,
                     {loc[0][g], loc[1][g], loc[2][g], loc[3][g], loc[4][g], loc[5][g]}, big_pref[bigsel],
                     {g ? nullptr : loc_pref[0], g ? nullptr : loc_pref[1], g ? nullptr : loc_pref[2],
                      g ? nullptr : loc_pref[3], g ? nullptr : loc_pref[4], g ? nullptr : loc_pref[5]}};
    }

    // room for `extra` more entries of the done list behind the ndone it holds
    int grow_done(uint64_t extra) {
        GK_TRY_HIP(c, grow_keep(c, "dn_start", ndone + extra, ndone, &dn_start));
        GK_TRY_HIP(c, grow_keep(c, "dn_len", ndone + extra, ndone, &dn_len));
        GK_TRY_HIP(c, grow_keep(c, "dn_par", ndone + extra, ndone, &dn_par));
        return GK_OK;
    }

    int init(uint64_t n_) {
        n = n_;
        GK_TRY_HIP(c, msd_tables());
        static_assert(4 * kCtrN <= 64 && 64 + 8 * kSumN <= 8 * kHostPinWords, "list counter block");
        uint64_t *cs;
        GK_TRY_HIP(c, scratch(c, "msd_ctr_sums", 8 + kSumN, &cs));
        ctr = reinterpret_cast<uint32_t *>(cs);
        sums = reinterpret_cast<unsigned long long *>(cs + 8);
        GK_TRY_HIP(c, hipMemsetAsync(ctr, 0, 4 * kCtrN, c->stream));
        const uint64_t max_big = n / kBlockMax + 2;
        GK_TRY_HIP(c, scratch(c, "big_start0", max_big, &big_start[0]));
        GK_TRY_HIP(c, scratch(c, "big_len0", max_big, &big_len[0]));
        GK_TRY_HIP(c, scratch(c, "big_start1", max_big, &big_start[1]));
        GK_TRY_HIP(c, scratch(c, "big_len1", max_big, &big_len[1]));
        GK_TRY_HIP(c, scratch(c, "big_pref0", max_big, &big_pref[0]));
        GK_TRY_HIP(c, scratch(c, "big_pref1", max_big, &big_pref[1]));
        if (int rc = grow_done(1024)) return rc;  // (ndone = 0: nothing kept)
        for (int k = 0; k < kLocal; ++k) GK_TRY_HIP(c, grow_keep(c, kLocName[k][0], 1024, 0, &loc[k][0]));
        for (int k = 0; k < kLocal; ++k) GK_TRY_HIP(c, grow_keep(c, kLocPrefName[k], 1024, 0, &loc_pref[k]));
        GK_TRY_HIP(c, scratch(c, "msd_heads", n + 64, &heads));
        return GK_OK;
    }

    // Keys of more than 64 bits are sorted in phases of one word (64 / bits symbols): phase 0 sorts
    // every k-mer by its first word, each later phase the groups of equal earlier words by the next
    int symbols_per_word() const { return 64 / ks.bits; }
    int phases() const { return (ks.symbols + symbols_per_word() - 1) / symbols_per_word(); }

    // The set-up of a sort entry point (all but msd_sort_groups, which sorts inside another sort's
    // product and neither writes final keys for the context nor takes packed-pair levels):
    //   B          the bits of the first key word (key_bits: keys that are not made of symbols)
    //   wkeys      a one-word sort ends with its keys final in keys[0] (*keys_final tells the entry point's caller)
    //              -- but the ACGT-only class of a mixed sba only where the split sort asks (acgt_keys)
    //   allow_c79  packed-pair levels where the bits fit
    // then the total timer, and the lists for n elements (kInitLater: n is not known yet)
    static constexpr uint64_t kInitLater = ~0ull;
    int begin(uint64_t n_, bool *keys_final, int key_bits = 0) {
        B = key_bits ? key_bits : ks.bits * std::min(ks.symbols, symbols_per_word());
        wkeys = (phases() == 1 && (!ks.acgt_only || acgt_keys)) ? 1 : 0;
        if (keys_final) *keys_final = wkeys != 0;
        allow_c79 = true;
        timer_begin(c, "msd_total", &total_slot);
        return n_ != kInitLater ? init(n_) : GK_OK;
    }

    // The L0 passes read the packed copy the transfer left beside the sba (gkm_xfer.hip: 0.37 B per
    // position instead of packing the bytes in every tile) where its stops are the k-mers' stops:
    // 2-bit keys, and the non-ACGT bytes are '$' alone (an ACGT sba) or all end the k-mers (the
    // ACGT-only class A of a mixed one).  Returns whether it is used.
    bool use_resident_pack() {
        if (!(c->res_pk && ks.bits == 2 && (c->acgt || ks.acgt_only))) return false;
        l0a.pk_code = c->res_code;
        l0a.pk_dol = c->res_dol;
        return true;
    }

    // the list counters and sums: one copy into pinned host memory
    int read_ctr() {
        uint64_t buf[8 + kSumN];
        GK_TRY_HIP(c, read_back(c, ctr, sizeof(buf), buf));
        std::memcpy(h, buf, 4 * kCtrN);
        std::memcpy(hs, buf + 8, 8 * kSumN);
        return GK_OK;
    }

    // scan per-tile histograms of nseg buckets (C chunks) into per-tile offsets + sub-bucket tables
    template <int RADIX>
    void scan_launch(uint64_t C, const uint32_t *s_cfirst, const uint32_t *s_nchunks, const uint32_t *s_start,
                     uint64_t nseg) {
        constexpr int TH = scan_threads<RADIX>();
        hipLaunchKernelGGL(chunk_sum_kernel<RADIX>, dim3((unsigned)C, RADIX / TH), dim3(TH), 0, c->stream, tile_hist,
                           c_first, c_ntiles, chunk_hist);
        hipLaunchKernelGGL(seg_scan_kernel<RADIX>, dim3((unsigned)nseg), dim3(TH), 0, c->stream, chunk_hist,
                           s_cfirst, s_nchunks, s_start, seg_base, seg_cnt);
        hipLaunchKernelGGL(tile_apply_kernel<RADIX>, dim3((unsigned)C, RADIX / TH), dim3(TH), 0, c->stream, tile_hist,
                           c_first, c_ntiles, chunk_hist);
    }

    int scan_offsets(int R, uint64_t C, const uint32_t *s_cfirst, const uint32_t *s_nchunks, const uint32_t *s_start,
                     uint64_t nseg) {
        timer_begin(c, "msd_scan", &slot);
        if (R == 8) scan_launch<256>(C, s_cfirst, s_nchunks, s_start, nseg);
        else if (R == 7) scan_launch<128>(C, s_cfirst, s_nchunks, s_start, nseg);
        else if (R == kWideL0) scan_launch<1 << kWideL0>(C, s_cfirst, s_nchunks, s_start, nseg);
        else scan_launch<64>(C, s_cfirst, s_nchunks, s_start, nseg);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        return GK_OK;
    }

    // tile / chunk tables: device buffers sized for T tiles, C chunks, nseg buckets
    int tables(uint64_t T, uint64_t C, uint64_t nseg) {
        const uint64_t rad = std::max(kGRadix, 1 << wsched[0]);  // the wide L0's digits
        GK_TRY_HIP(c, scratch(c, "tile_hist", T * rad, &tile_hist));
        GK_TRY_HIP(c, scratch(c, "chunk_hist", C * rad, &chunk_hist));
        GK_TRY_HIP(c, scratch(c, "c_first", C, &c_first));
        GK_TRY_HIP(c, scratch(c, "c_ntiles", C, &c_ntiles));
        GK_TRY_HIP(c, scratch(c, "seg_base", nseg * rad, &seg_base));
        GK_TRY_HIP(c, scratch(c, "seg_cnt", nseg * rad, &seg_cnt));
        return GK_OK;
    }

    // a persistent grid: the workgroups of `fn` that are resident at once, at most one per item of work
    unsigned resident_grid(const void *fn, int threads, uint64_t work) {
        return (unsigned)std::min<uint64_t>(work, (uint64_t)cus * resident_per_cu(c, fn, threads));
    }

    // a key-range rank's compacting L0 over the packed copy (l0_dispatch_c, GKM_OWN_L0_COMPACT=1):
    // count, or partition into packed (pk) or plain output
    template <int R>
    void own_launch(bool count, bool pk, const L0Args &a, Dig d0, const OwnTest &ot, unsigned nt0, uint64_t *kout,
                    uint32_t *vout, uint32_t nt, const NextDigits &ndg) {
        if (count)
            hipLaunchKernelGGL(own_count_kernel<R>, dim3(resident_grid((const void *)own_count_kernel<R>, kOwnT, nt0)),
                               dim3(kOwnT), 0, c->stream, a, d0, ot, tile_hist, nt0);
        else if (pk)
            hipLaunchKernelGGL((own_part_kernel<R, true>),
                               dim3(resident_grid((const void *)own_part_kernel<R, true>, kOwnT, nt0)), dim3(kOwnT), 0,
                               c->stream, a, d0, ot, tile_hist, kout, vout, nt, ndg);
        else
            hipLaunchKernelGGL((own_part_kernel<R, false>),
                               dim3(resident_grid((const void *)own_part_kernel<R, false>, kOwnT, nt0)), dim3(kOwnT), 0,
                               c->stream, a, d0, ot, tile_hist, kout, vout, nt, ndg);
    }

    // L0 kernels: count (per-tile digit histograms) or partition; bits x digit width x next digits
    // x canonical
    template <int BITS, int R, bool ND, bool CANON, bool P88 = false, bool OWN = false>
    void l0_launch(bool count, const L0Args &a, Dig d0, unsigned nt0, uint64_t *kout, uint32_t *vout, uint32_t nt,
                   uint64_t sink, const NextDigits &ndg) {
        // the count pass streams the sequence: 256-thread workgroups, eight per CU, each holding a
        // whole tile of loads in flight (1,024-thread ones, two per CU, kept a quarter as many
        // bytes in flight and measured slower)
        if (count)
            hipLaunchKernelGGL((msd0_count_kernel<BITS, kP0T / 4, kP0I * 4, R, CANON>),
                               dim3(resident_grid((const void *)msd0_count_kernel<BITS, kP0T / 4, kP0I * 4, R, CANON>,
                                                  kP0T / 4, nt0)),
                               dim3(kP0T / 4), 0, c->stream, a, d0, tile_hist, nt0);
        else
            hipLaunchKernelGGL((msd0_pipe_kernel<BITS, kP0T, kP0I, R, ND, CANON, P88, OWN>), dim3(pgrid), dim3(kP0T),
                               0, c->stream, a, d0, tile_hist, kout, vout, nt, sink, ndg);
    }

    template <bool CANON>
    void l0_dispatch_c(bool count, int w0, bool nd_, const L0Args &a, Dig d0, unsigned nt0, uint64_t *kout,
                       uint32_t *vout, uint32_t nt, uint64_t sink, const NextDigits &ndg) {
        if (ks.bits == 2 && !CANON && w0 == kWideL0) {  // enable_wide_l0: forward 2-bit one-word sorts
            if (count)
                hipLaunchKernelGGL((msd0_count_kernel<2, 256, kWT * kWI / 256, kWideL0, false>),
                                   dim3(resident_grid(
                                       (const void *)msd0_count_kernel<2, 256, kWT * kWI / 256, kWideL0, false>, 256, nt0)),
                                   dim3(256), 0, c->stream, a, d0, tile_hist, nt0);
            else if (nd_)
                hipLaunchKernelGGL((msd0_wide_kernel<kWT, kWI, kWideL0, true>), dim3(pgrid), dim3(kWT), 0, c->stream,
                                   a, d0, tile_hist, kout, vout, nt, sink, ndg);
            else
                hipLaunchKernelGGL((msd0_wide_kernel<kWT, kWI, kWideL0, false>), dim3(pgrid), dim3(kWT), 0,
                                   c->stream, a, d0, tile_hist, kout, vout, nt, sink, ndg);
            return;
        }
        const bool pk = !count && nd_ && ndg.out16 != nullptr;  // the packed L0 (P88)
        // a key-range rank's L0 over the packed copy: test, compact, then rank only the kept k-mers
        // (GKM_OWN_L0_COMPACT=1, measured slower than the select + level from pieces at N >= 4 and
        // equal to the tile L0 at N = 2: own_part_kernel)
        if (ks.bits == 2 && !CANON && a.own_span != 0xFFFFFFFFu && a.own_span != 0 && a.pk_code &&
            ks.symbols <= 32 && a.own_bits <= 32 && (w0 == 7 || w0 == kGR) && (count || nd_) &&
            opt("GKM_OWN_L0_COMPACT")) {
            const int sh = 32 - a.own_bits;
            const OwnTest ot{(uint32_t)((uint64_t)a.own_lo << sh),
                             (uint32_t)(((uint64_t)std::min<uint64_t>(a.own_span, 1ull << a.own_bits) << sh) - 1)};
            if (w0 == 7) own_launch<7>(count, pk, a, d0, ot, nt0, kout, vout, nt, ndg);
            else own_launch<kGR>(count, pk, a, d0, ot, nt0, kout, vout, nt, ndg);
            return;
        }
        if (!count && ks.bits == 2 && nd_ && a.own_span != 0xFFFFFFFFu) {  // a key-range rank's fused select
            if (w0 == 7) {
                if (pk) l0_launch<2, 7, true, CANON, true, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
                else l0_launch<2, 7, true, CANON, false, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            } else {
                if (pk) l0_launch<2, kGR, true, CANON, true, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
                else l0_launch<2, kGR, true, CANON, false, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            }
            return;
        }
        if (ks.bits == 2 && w0 == 7) {
            if (pk) l0_launch<2, 7, true, CANON, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else if (nd_) l0_launch<2, 7, true, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else l0_launch<2, 7, false, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
        } else if (ks.bits == 2 && w0 == 6 && !CANON) {  // (A/B, GKM_LEVEL_BITS=6,...: half the L0's write streams)
            if (pk) l0_launch<2, 6, true, false, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else if (nd_) l0_launch<2, 6, true, false>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else l0_launch<2, 6, false, false>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
        } else if (ks.bits == 2) {
            if (pk) l0_launch<2, kGR, true, CANON, true>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else if (nd_) l0_launch<2, kGR, true, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else l0_launch<2, kGR, false, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
        } else {
            if (nd_) l0_launch<4, kGR, true, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
            else l0_launch<4, kGR, false, CANON>(count, a, d0, nt0, kout, vout, nt, sink, ndg);
        }
    }

    void l0_dispatch(bool count, int w0, bool nd_, const L0Args &a, Dig d0, unsigned nt0, uint64_t *kout,
                     uint32_t *vout, uint32_t nt, uint64_t sink, const NextDigits &ndg) {
        if (ks.canonical) l0_dispatch_c<true>(count, w0, nd_, a, d0, nt0, kout, vout, nt, sink, ndg);
        else l0_dispatch_c<false>(count, w0, nd_, a, d0, nt0, kout, vout, nt, sink, ndg);
    }

    // L0: the k-mers starting in [lo, hi) encoded and partitioned by their top width(0) key bits, in
    // two passes over the sequence.  Key-range shards keep only the k-mers whose ownership digit
    // (the top own_bits key bits) is in [own_lo, own_lo + own_span); all owned: 0, 0xFFFFFFFF.
    //
    // L0 count pass: per-tile digit histograms of the kept k-mers starting in [lo, hi), their
    // column scan (seg_base / seg_cnt then hold the 2^width(0) buckets), *count = k-mers kept
    int l0_count(uint64_t lo, uint64_t hi, uint32_t own_lo, uint32_t own_span, uint64_t *count, int own_bits = 0) {
        const uint64_t span = hi > lo ? hi - lo : 0;
        const uint64_t tile = wsched[0] == kWideL0 ? (uint64_t)kWT * kWI : (uint64_t)kP0Tile;  // (the wide L0's own)
        const uint64_t nt0 = std::max<uint64_t>((span + tile - 1) / tile, 1);
        const uint64_t nc0 = (nt0 + ctiles - 1) / ctiles;
        l0_tiles = nt0;
        int rc = tables(nt0, nc0, 1);
        if (rc != GK_OK) return rc;
        uint32_t *s_misc;
        GK_TRY_HIP(c, scratch(c, "s_misc", 4, &s_misc));
        {
            std::vector<uint32_t> cf(nc0), cn(nc0);
            for (uint64_t j = 0; j < nc0; ++j) {
                cf[j] = (uint32_t)(j * ctiles);
                cn[j] = (uint32_t)std::min<uint64_t>(ctiles, nt0 - j * ctiles);
            }
            const uint32_t misc[3] = {0, (uint32_t)nc0, 0};  // s_cfirst, s_nchunks, s_start
            GK_TRY_HIP(c, hipMemcpyAsync(c_first, cf.data(), 4 * nc0, hipMemcpyHostToDevice, c->stream));
            GK_TRY_HIP(c, hipMemcpyAsync(c_ntiles, cn.data(), 4 * nc0, hipMemcpyHostToDevice, c->stream));
            GK_TRY_HIP(c, hipMemcpyAsync(s_misc, misc, 12, hipMemcpyHostToDevice, c->stream));
            GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        }
        L0Args a{c->sba, lo, hi, ks.symbols, B, ks.acgt_only};
        a.own_lo = own_lo;
        a.own_span = own_span;
        if (own_bits) a.own_bits = own_bits;
        a.pk_code = l0a.pk_code;
        a.pk_dol = l0a.pk_dol;
        l0a = a;
        const int w0 = width(0);
        const Dig d0 = dig_at(B, 0, w0);
        timer_begin(c, "msd_l0_count", &slot);
        l0_dispatch(true, w0, false, a, d0, (unsigned)nt0, nullptr, nullptr, 0, 0, NextDigits{});
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        rc = scan_offsets(w0, nc0, s_misc, s_misc + 1, s_misc + 2, 1);
        if (rc != GK_OK) return rc;
        // the bucket total = k-mers found (the last bucket's base + count)
        uint32_t last[2];
        GK_TRY_HIP(c, hipMemcpyAsync(&last[0], seg_base + (1 << w0) - 1, 4, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(&last[1], seg_cnt + (1 << w0) - 1, 4, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        *count = (uint64_t)last[0] + last[1];
        return GK_OK;
    }

    // L0 partition pass after l0_count (same tiles, same range) into kout / vout (capacity >=
    // count + 1: element `count` is the scatter's sink)
    int l0_partition(uint64_t *kout, uint32_t *vout, uint64_t cap, uint64_t count) {
        if (count + 1 > cap) return fail(c, GK_E_ARG, "partition output buffer too small");
        const int w0 = width(0);
        const Dig d0 = dig_at(B, 0, w0);
        timer_begin(c, p88 ? "msd_pass_l0k" : "msd_pass_l0", &slot);  // (l0k: the packed L0 output)
        timer_units(c, slot, count);
        // the sort's own L0 also writes the level-1 digits (shard sends are re-counted after the
        // exchange, so they do not)
        // (a starts-only shard send has no key output: kout == nullptr, which a context whose key
        // buffers are not allocated yet must not mistake for one of them)
        const bool with_nd = kout && (kout == c->keys[0] || kout == c->keys[1]);
        NextDigits ndg{dig_at(B, w0, width(1)), nullptr};
        if (with_nd && p88) {  // the packed L0: digit bytes and low start bits in the free start buffer
            p88_place(vout == c->vals[0] ? 0 : 1);
            nd = nd_l0;
            ndg.out = nd;
            ndg.out16 = lo16_l0;
            ndg.pshi = p88_shi;
        } else if (with_nd) {
            GK_TRY_HIP(c, scratch(c, "msd_nd", n + 64, &nd));
            ndg.out = nd;
        }
        l0_dispatch(false, w0, with_nd, l0a, d0, (unsigned)l0_tiles, kout, vout, (uint32_t)l0_tiles, count, ndg);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        cur_fmt = !with_nd ? Fmt::KeyStart : p88 ? Fmt::PackedL0 : Fmt::KeyStartDigit;
        return GK_OK;
    }

    // the packed L0 pays when the level behind it writes packed pairs itself (it reads the packed
    // form, INP = 2): the same prediction level_pass makes at L1 from the mean bucket sizes, with the
    // L1 digit being the digit byte (8 bits).  GKM_TEST_P88=1 (tests): wherever
    // the bits fit.  C3: 62 - 7 = 55 bits after the L0, 47 of them in the pair (shi 17).
    bool p88_wanted() const {
        if (!allow_c79 || ks.bits != 2 || phase != 0 || no_compact()) return false;
        const int w0 = width(0), w1 = width(1), w2 = width(2), rem = B - w0;
        if ((w0 != 6 && w0 != 7 && w0 != kGR) || w1 != 8 || rem - 8 < 33 || rem - 8 > 48) return false;
        if (opt("GKM_TEST_P88")) return true;
        const uint64_t m1 = (n >> w0) >> w1;  // mean L1 sub-bucket
        const int rem2 = rem - w1 - w2;
        return m1 >= (uint64_t)kBlockMax && (m1 >> w2) < (uint64_t)kBlockMax && rem2 >= 9 && rem2 <= 40 && w2 == 8 &&
               width(3) == 8;
    }

    // The packed L0 writes no starts, so its low start bits and digit bytes live in the start buffer
    // of its own output (vals[buf]: 4 B per element; 2 + 1 used) -- no extra memory.  An expansion
    // back to (key, start) writes that buffer, so it first copies them out (p88_detach, rare: skewed
    // genomes and test shapes) and every later reader takes the copy.
    void p88_place(int buf) {
        lo16_l0 = reinterpret_cast<uint16_t *>(c->vals[buf]);
        nd_l0 = reinterpret_cast<uint8_t *>(c->vals[buf]) + ((2 * (c->elem_cap + 64) + 255) & ~255ull);
    }
    int p88_detach() {
        uint8_t *t;
        const uint64_t m = c->elem_cap + 64;
        if (!lo16_l0) return GK_OK;
        GK_TRY_HIP(c, scratch(c, "p88_detached", 3 * m, &t));
        if (reinterpret_cast<uint8_t *>(lo16_l0) == t) return GK_OK;  // (already)
        GK_TRY_HIP(c, hipMemcpyAsync(t, lo16_l0, 2 * m, hipMemcpyDeviceToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(t + 2 * m, nd_l0, m, hipMemcpyDeviceToDevice, c->stream));
        if (nd == nd_l0) nd = t + 2 * m;
        lo16_l0 = reinterpret_cast<uint16_t *>(t);
        nd_l0 = t + 2 * m;
        return GK_OK;
    }

    // after the packed L0's classify: its local entries back to (key, start) for the finishing kernels
    int expand_p88_locals(int buf) {
        bool any = false;
        for (int k = 0; k < kLocal; ++k) any |= nloc[k] > 0;
        if (!any) return GK_OK;
        if (int rc = p88_detach()) return rc;
        for (int k = 0; k < kLocal; ++k) {
            if (!nloc[k]) continue;
            hipLaunchKernelGGL(expand_p88_list_kernel, dim3((unsigned)nloc[k]), dim3(256), 0, c->stream, loc[k][0],
                               loc_pref[k], B, p88_shi, c->keys[buf], lo16_l0, nd_l0, c->vals[buf]);
            GK_TRY_HIP(c, hipGetLastError());
        }
        return GK_OK;
    }

    // The start of a sort from the sequence, behind l0_count (which found the n = `found` k-mers this
    // sort keeps) and init(found): the L0 partition into the buffer *in, its buckets routed.
    int l0_start(uint64_t found, int *in) {
        // the packed L0 output (P88) when the level behind it writes packed pairs
        p88 = p88_wanted();  // (multi-word keys: phase 0's first word; the tie phases read keys[0] / vals[0])
        p88_shi = 64 - (B - width(0) - 8);
        // The L0's output buffer: the one that makes the last global level write buffer 1, so that the
        // finishing kernels read buffer 1 and write buffer 0 instead of rewriting buffer 0 in place
        // (levels predicted from the mean bucket size; C3: L0, L1, L2 -> L0 writes buffer 1).  A/B on
        // one box (C3, 3 pairs): 67.3-68.3 against 67.7-68.8 ms.
        uint64_t mean = found >> width(0);
        int lev = 0;
        for (int l = 1; mean > (uint64_t)kBlockMax && l < kMaxLevels; ++l, ++lev) mean >>= width(l);
        const int l0b = 1 ^ (lev & 1);
        *in = l0b;
        int rc = l0_partition(c->keys[l0b], c->vals[l0b], c->elem_cap + 64, found);
        if (rc != GK_OK) return rc;
        rc = classify(1u << width(0), width(0), l0b, 0, nullptr, nullptr, 1, nullptr, width(0));
        if (rc != GK_OK) return rc;
        return cur_fmt == Fmt::PackedL0 ? expand_p88_locals(l0b) : GK_OK;  // (skewed genomes: L0 buckets finished locally)
    }

    // one region of the prefetched L0 (L0Prefetch, below): count, column scan and partition of the
    // k-mers starting in [lo, hi) into keys[1] / vals[1] / nd at output indices from lo, then the
    // region's 2^w0 bucket bases and counts into `pieces` -- all on c->stream (the caller points it
    // at the prefetch stream), with the region's chunk tables already in `tab` (c_first[nc],
    // c_ntiles[nc], then s_cfirst, s_nchunks, s_start) and no host round trip
    int l0_region(uint64_t lo, uint64_t hi, uint32_t nt, uint32_t nc, uint32_t nc_max, uint32_t *tab, uint64_t sink,
                  uint32_t *pieces) {
        int rc = tables(nt, nc, 1);  // (allocated by prefetch_plan: no reallocation here)
        if (rc != GK_OK) return rc;
        c_first = tab;  // (the region's table: nc_max entries each, then misc)
        c_ntiles = tab + nc_max;
        const uint32_t *misc = tab + 2 * nc_max;
        // (acgt_only: every byte other than A/C/G/T ends k-mers -- on an ACGT sba exactly the '$'
        // separators, so this is the plain sort's L0 there, and the class-A L0 of a mixed sba's
        // split sort elsewhere)
        const L0Args a{c->sba, lo, hi, ks.symbols, B, 1};
        const int w0 = width(0);
        const Dig d0 = dig_at(B, 0, w0);
        l0_dispatch(true, w0, false, a, d0, nt, nullptr, nullptr, 0, 0, NextDigits{});
        GK_TRY_HIP(c, hipGetLastError());
        rc = scan_offsets(w0, nc, misc, misc + 1, misc + 2, 1);
        if (rc != GK_OK) return rc;
        NextDigits ndg{dig_at(B, w0, width(1)), nd};
        if (p88) {  // the packed L0 (P88): nd / lo16_l0 set by the caller
            ndg.out16 = lo16_l0;
            ndg.pshi = p88_shi;
        }
        l0_dispatch(false, w0, true, a, d0, nt, c->keys[1], c->vals[1], nt, sink, ndg);
        GK_TRY_HIP(c, hipGetLastError());
        GK_TRY_HIP(c, hipMemcpyAsync(pieces, seg_base, 4u << w0, hipMemcpyDeviceToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(pieces + (1u << w0), seg_cnt, 4u << w0, hipMemcpyDeviceToDevice, c->stream));
        return GK_OK;
    }

    // after a compact level: the (rare) sub-buckets that go to another global level get their keys
    // back in keys[out], so that level reads keys as usual (the digit bytes stay valid for it)
    int expand_big(int out) {
        if (cur_fmt != Fmt::Compact || nbig == 0) return GK_OK;
        hipLaunchKernelGGL(expand_compact_kernel, dim3(nbig, bucket_split(nbig)), dim3(256), 0, c->stream, big_start[cur_big],
                           big_len[cur_big], big_pref[cur_big], compact_hi, B, nd, c->keys[out], c->vals[out]);
        GK_TRY_HIP(c, hipGetLastError());
        return GK_OK;
    }

    // route nsub sub-buckets (seg_base / seg_cnt, or base / cnt) of a level; hi = key bits sorted
    // after it; sub-buckets under min_size elements are dropped (final as they stand)
    // ppref / pw / compact: see classify_kernel
    int classify(uint64_t nsub, int hi, int parity, int bigsel, const uint32_t *base = nullptr,
                 const uint32_t *cnt = nullptr, uint32_t min_size = 1, const uint64_t *ppref = nullptr, int pw = 0,
                 int compact = 0, bool read = true) {
        if (!base) base = seg_base;
        if (!cnt) cnt = seg_cnt;
        for (int k = 0; k < kLocal; ++k)
            GK_TRY_HIP(c, grow_keep(c, kLocName[k][0], nloc[k] + nsub, nloc[k], &loc[k][0]));
        for (int k = 0; k < kLocal; ++k)
            GK_TRY_HIP(c, grow_keep(c, kLocPrefName[k], nloc[k] + nsub, nloc[k], &loc_pref[k]));
        if (int rc = grow_done(nsub)) return rc;
        GK_TRY_HIP(c, hipMemsetAsync(ctr + kCtrBig, 0, 4, c->stream));
        GK_TRY_HIP(c, hipMemsetAsync(sums, 0, 8 * kSumN, c->stream));
        timer_begin(c, "msd_classify", &slot);
        hipLaunchKernelGGL(classify_kernel, dim3((unsigned)((nsub + kClassT - 1) / kClassT)), dim3(kClassT), 0,
                           c->stream, base, cnt, nsub, hi, B, parity, lists(0, bigsel), ctr, sums, min_size, ppref, pw,
                           compact, (uint32_t)kPTile, ctiles);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        return read ? classify_counts() : GK_OK;
    }

    // the lists classify wrote (and route_uniform's device-count path re-routed), to the host: only
    // behind a classify that did not read back itself (loc_elems is added to)
    int classify_counts() {
        int r = read_ctr();
        if (r != GK_OK) return r;
        for (int k = 0; k < kLocal; ++k) {
            nloc[k] = h[kCtrLoc + k];
            loc_elems[k] += hs[kCtrLoc + k];
        }
        ndone = h[kCtrDone];
        nbig = h[kCtrBig];
        big_elems = hs[kCtrBig];
        return GK_OK;
    }

    // Before another global level: the buckets of the next-level list whose keys are all equal go to
    // the done list, the others to the other next-level list (keys in keys[out]).  Two callers:
    //   dev_count = false  behind a classify that read its lists: nb = nbig, exact grids, and only
    //       what this changes is read back (ndone, nbig, big_elems).  NOT classify_counts: that adds
    //       the local lists' element sums to loc_elems, which the classify's read already did.
    //   dev_count = true   behind a classify that did not read back (the deep levels of a repeat-rich
    //       genome: one host round trip per level instead of two): the list's count stays on the
    //       device, nb >= that count sizes the grids (the blocks past the count return at once), a
    //       compact level's buckets get their keys back here (the host path's expand_big), and the
    //       one read-back is the classify's own (classify_counts).
    int route_uniform(int out, uint32_t nb, bool dev_count) {
        const uint32_t *nb_dev = dev_count ? ctr + kCtrBig : nullptr;
        uint32_t *nb_copy = dev_count ? ctr + kCtrNbCopy : nullptr;  // (the flag kernel's copy: kCtrBig is reset)
        const unsigned split = bucket_split(nb);
        if (dev_count && cur_fmt == Fmt::Compact)
            hipLaunchKernelGGL(expand_compact_kernel, dim3(nb, split), dim3(256), 0, c->stream, big_start[cur_big],
                               big_len[cur_big], big_pref[cur_big], compact_hi, B, nd, c->keys[out], c->vals[out],
                               nb_dev);
        uint32_t *mixed;
        GK_TRY_HIP(c, scratch(c, "uni_mixed", nb, &mixed));
        GK_TRY_HIP(c, hipMemsetAsync(mixed, 0, 4ull * nb, c->stream));
        hipLaunchKernelGGL(uniform_flag_kernel, dim3(nb, split), dim3(256), 0, c->stream, big_start[cur_big],
                           big_len[cur_big], c->keys[out], mixed, nb_dev, nb_copy);
        // (dev_count: the done list has room -- the classify grew it by every sub-bucket, and each
        // goes to one list)
        if (!dev_count)
            if (int rc = grow_done(nb)) return rc;
        GK_TRY_HIP(c, hipMemsetAsync(ctr + kCtrBig, 0, 4, c->stream));
        GK_TRY_HIP(c, hipMemsetAsync(sums + kCtrBig, 0, 8, c->stream));
        GK_TRY_HIP(c, hipMemsetAsync(sums + kSumTiles, 0, 16, c->stream));
        hipLaunchKernelGGL(route_uniform_kernel, dim3(grid256_min1(nb)), dim3(256), 0, c->stream, big_start[cur_big],
                           big_len[cur_big], big_pref[cur_big], nb, mixed, lists(0, cur_big ^ 1), out, ctr, sums,
                           (uint32_t)kPTile, ctiles, nb_copy);
        GK_TRY_HIP(c, hipGetLastError());
        cur_big ^= 1;
        if (dev_count) return classify_counts();
        int r = read_ctr();
        if (r != GK_OK) return r;
        ndone = h[kCtrDone];
        nbig = h[kCtrBig];
        big_elems = hs[kCtrBig];
        return GK_OK;
    }

    // route_uniform pays once the next-level buckets hold few elements: after L1 of a random genome
    // they hold all of them and are never uniform (`elems`: the level's output, or its input where
    // the decision comes before the classify's read-back)
    bool few_big_elems(int level, uint64_t elems) const {
        return level >= 1 && elems * 64 <= std::max<uint64_t>(n, 1);
    }

    // Which input format a level writing `out` reads as it is; any other input goes back to (key,
    // start) + digit bytes first, by the expand_* launches of whoever holds the buckets (level_pass:
    // the next-level list; first_level_from_pieces: the pieces).
    static bool reads(Fmt in, Fmt out) {
        switch (in) {
        case Fmt::Pairs: return out == Fmt::Compact;    // (msd_pipe_kernel<..., 4, ., ., IN79>)
        case Fmt::PackedL0: return out == Fmt::Pairs;   // (msd_pipe_kernel<..., 5, ., ., INP = 2>)
        default: return true;  // keys and starts (a compact level's large buckets: expand_big made them so)
        }
    }
    bool has_digits() const { return cur_fmt != Fmt::KeyStart; }

    // one global partition level (R-bit digits below the top hi bits) over tiles already in
    // t_start / t_count (T tiles, C chunks, nseg buckets), reading kin / vin (format cur_fmt), writing
    // keys[out] / vals[out] in format ofmt
    template <int R>
    void level_launch(int hi, int nw, const uint32_t *t_start, const uint32_t *t_count, uint64_t T,
                      const uint64_t *kin, const uint32_t *vin, int out, bool count, Fmt ofmt) {
        if (count) {
            if (has_digits())  // the previous pass wrote this level's digits
                hipLaunchKernelGGL(msd_count_nd_kernel<R>, dim3((unsigned)T), dim3(256), 0, c->stream, t_start,
                                   t_count, nd, tile_hist);
            else
                hipLaunchKernelGGL(msd_count_kernel<R>, dim3((unsigned)T), dim3(256), 0, c->stream, t_start, t_count,
                                   dig_at(B, hi, R), kin, tile_hist);
            return;
        }
        if (ofmt == Fmt::Compact) {
            const int rem = B - hi - R;  // 9..40: key bits below this level's digit
            NextDigits ndg{dig_at(B, hi + R, 8), nd};
            ndg.lowmask = (uint32_t)((1ull << (rem - 8)) - 1);
            if (cur_fmt == Fmt::Pairs)  // the previous level wrote packed pairs
                hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 4, true, 0, true>), dim3(pgrid), dim3(kPT), 0,
                                   c->stream, t_start, t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out],
                                   c->vals[out], (uint32_t)T, n, ndg, lo16, c79_shi);
            else
                hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 4, true>), dim3(pgrid), dim3(kPT), 0, c->stream,
                                   t_start, t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out],
                                   c->vals[out], (uint32_t)T, n, ndg);
            return;
        }
        if (ofmt == Fmt::Pairs) {  // packed pairs for the compact level behind this one
            NextDigits ndg{dig_at(B, hi + R, nw), nd};
            ndg.out16 = lo16;
            ndg.pshi = c79_shi;
            if (cur_fmt == Fmt::PackedL0) {  // reading the packed L0's output
                ndg.in8 = nd_l0;
                hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 5, true, 0, 2>), dim3(pgrid), dim3(kPT), 0, c->stream,
                                   t_start, t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out], c->vals[out],
                                   (uint32_t)T, n, ndg, lo16_l0, p88_shi);
                return;
            }
            hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 5, true>), dim3(pgrid), dim3(kPT), 0, c->stream, t_start,
                               t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out], c->vals[out],
                               (uint32_t)T, n, ndg);
            return;
        }
        const NextDigits ndg{dig_at(B, hi + R, nw), nd};
        if (ofmt == Fmt::KeyStartDigit)
            hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 0, true>), dim3(pgrid), dim3(kPT), 0, c->stream, t_start,
                               t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out], c->vals[out],
                               (uint32_t)T, n, ndg);
        else
            hipLaunchKernelGGL((msd_pipe_kernel<kPT, kPI, R, 0, false>), dim3(pgrid), dim3(kPT), 0, c->stream,
                               t_start, t_count, dig_at(B, hi, R), tile_hist, kin, vin, c->keys[out], c->vals[out],
                               (uint32_t)T, n, ndg);
    }

    void level_dispatch(int level, int hi, const uint32_t *t_start, const uint32_t *t_count, uint64_t T,
                        const uint64_t *kin, const uint32_t *vin, int out, bool count, Fmt ofmt) {
        const int w = width(level), nw = width(level + 1);
        if (w == 8) level_launch<8>(hi, nw, t_start, t_count, T, kin, vin, out, count, ofmt);
        else if (w == 7) level_launch<7>(hi, nw, t_start, t_count, T, kin, vin, out, count, ofmt);
        else level_launch<6>(hi, nw, t_start, t_count, T, kin, vin, out, count, ofmt);
    }

    // the output format of a global level over nseg buckets holding elems elements, reading cur_fmt:
    //   KeyStartDigit  the next level's digit bytes are written too (its sub-buckets are most likely
    //                  big); KeyStart otherwise: a next level then counts from the keys;
    //   Compact  (low bits, start) + digit byte, 9 B out, when its sub-buckets will most likely all
    //            be finished locally and the key bits below the next 8-bit digit fit a u32;
    //   Pairs    packed pairs (10 B + digit byte) when the next level is most likely compact (its
    //            sub-buckets local, its remaining bits <= 40) and this level's remaining key bits
    //            and the start fit 80 bits (GKM_TEST_PAIRS=1, tests: whenever the bits fit)
    Fmt level_format(int level, int hi, uint64_t elems, uint64_t nseg) const {
        const bool digits = nseg == 0 || (elems / nseg >> width(level)) >= (uint64_t)kBlockMax;
        const int rem = B - hi - width(level);
        if (phase == 0 && !digits && rem >= 9 && rem <= 40 && width(level + 1) == 8 && !no_compact())
            return Fmt::Compact;
        const uint64_t next_mean = nseg ? (elems / nseg >> width(level)) >> width(level + 1) : 0;
        const int rem2 = rem - width(level + 1);
        const bool force = opt("GKM_TEST_PAIRS") != nullptr;  // (read per level: tests flip it)
        if (allow_c79 && cur_fmt != Fmt::Pairs && phase == 0 && rem >= 33 && rem <= 48 && !no_compact() &&
            (force || (digits && next_mean < (uint64_t)kBlockMax && rem2 >= 9 && rem2 <= 40 &&
                       width(level + 2) == 8 && width(level + 1) == 8)))
            return Fmt::Pairs;
        return digits ? Fmt::KeyStartDigit : Fmt::KeyStart;
    }

    int level_pass(int level, int hi, const uint32_t *t_start, const uint32_t *t_count, uint64_t T, uint64_t C,
                   const uint32_t *s_cfirst, const uint32_t *s_nchunks, const uint32_t *s_start, uint64_t nseg,
                   const uint64_t *kin, const uint32_t *vin, int out) {
        timer_begin(c, has_digits() ? "msd_count_nd" : "msd_count", &slot);
        timer_units(c, slot, big_elems);
        level_dispatch(level, hi, t_start, t_count, T, kin, vin, out, true, cur_fmt);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        int rc = scan_offsets(width(level), C, s_cfirst, s_nchunks, s_start, nseg);
        if (rc != GK_OK) return rc;
        GK_TRY_HIP(c, scratch(c, "msd_nd", n + 64, &nd));
        const Fmt ofmt = level_format(level, hi, big_elems, nseg);
        compact_hi = hi + width(level);
        const int rem = B - hi - width(level);
        if (ofmt == Fmt::Pairs) {
            c79_shi = 64 - rem;
            GK_TRY_HIP(c, scratch(c, "msd_lo16", n + 64, &lo16));
        }
        if (!reads(cur_fmt, ofmt)) {  // back to (key, start) first; the digit bytes stay
            if (cur_fmt == Fmt::PackedL0) {
                if (int rc = p88_detach()) return rc;
                hipLaunchKernelGGL(expand_p88_kernel, dim3((unsigned)nseg, bucket_split(nseg)), dim3(256), 0,
                                   c->stream, big_start[cur_big], big_len[cur_big], big_pref[cur_big], hi, B, p88_shi,
                                   const_cast<uint64_t *>(kin), lo16_l0, nd_l0, const_cast<uint32_t *>(vin));
            } else {  // Pairs
                hipLaunchKernelGGL(expand_pair_kernel, dim3((unsigned)nseg, bucket_split(nseg)), dim3(256), 0,
                                   c->stream, big_start[cur_big], big_len[cur_big], big_pref[cur_big], hi, B, c79_shi,
                                   const_cast<uint64_t *>(kin), lo16, const_cast<uint32_t *>(vin));
            }
            GK_TRY_HIP(c, hipGetLastError());
            cur_fmt = Fmt::KeyStartDigit;
        }
        timer_begin(c, ofmt == Fmt::Compact ? kPassNamesC[level & 7] : ofmt == Fmt::Pairs ? kPassNamesP[level & 7]
                                                                                          : kPassNames[level & 7],
                    &slot);
        timer_units(c, slot, big_elems);
        level_dispatch(level, hi, t_start, t_count, T, kin, vin, out, false, ofmt);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        // (a compact or packed-pair level wrote the next 8-bit digit too: the next count must not
        // read keys -- pairs hold them shifted)
        cur_fmt = ofmt;
        return GK_OK;
    }

    // after a packed-pair level's classify: its local buckets (entries [before[k], nloc[k]) of the
    // generation-0 lists) back to (key, start) for the finishing kernels
    int expand_pair_locals(const uint64_t (&before)[kLocal], int out) {
        for (int k = 0; k < kLocal; ++k) {
            if (nloc[k] <= before[k]) continue;
            hipLaunchKernelGGL(expand_pair_list_kernel, dim3((unsigned)(nloc[k] - before[k])), dim3(256), 0,
                               c->stream, loc[k][0], loc_pref[k], (uint32_t)before[k], B, c79_shi, c->keys[out], lo16,
                               c->vals[out]);
            GK_TRY_HIP(c, hipGetLastError());
        }
        return GK_OK;
    }

    // first level from received buckets: pieces (off, len) of kin / vin, grouped by top-kGR-bit
    // bucket in ascending bucket order, pieces of a bucket in the order their elements must keep
    // level / hi: the level the pieces are partitioned at and the key bits already sorted (the
    // exchange's pieces: level 1 after kGR bits; the key-range select's chunks: level 0, no bits)
    int first_level_from_pieces(const uint64_t *kin, const uint32_t *vin, const uint64_t *poff, const uint64_t *plen,
                                const uint32_t *pbucket, uint32_t np, int level = 1, int hi = kGR) {
        std::vector<uint32_t> ts, tc, cf, cn, scf, snc, sst;
        std::vector<uint64_t> spf;  // the buckets' prefixes: their top-hi-bit values
        uint64_t out_base = 0;
        for (uint32_t i = 0; i < np;) {
            uint32_t j = i;
            uint64_t tot = 0;
            const uint64_t tile0 = ts.size();
            while (j < np && pbucket[j] == pbucket[i]) {
                for (uint64_t o = 0; o < plen[j]; o += kPTile) {
                    ts.push_back((uint32_t)(poff[j] + o));
                    tc.push_back((uint32_t)std::min<uint64_t>(kPTile, plen[j] - o));
                }
                tot += plen[j];
                ++j;
            }
            if (tot > 0) {
                const uint64_t nt = ts.size() - tile0;
                scf.push_back((uint32_t)cf.size());
                for (uint64_t t = 0; t < nt; t += ctiles) {
                    cf.push_back((uint32_t)(tile0 + t));
                    cn.push_back((uint32_t)std::min<uint64_t>(ctiles, nt - t));
                }
                snc.push_back((uint32_t)(cf.size() - scf.back()));
                sst.push_back((uint32_t)out_base);
                spf.push_back(pbucket[i]);
                out_base += tot;
            }
            i = j;
        }
        if (out_base != n) return fail(c, GK_E_ARG, "piece lengths do not add up to n");
        const uint64_t T = ts.size(), C = cf.size(), nseg = sst.size();
        if (nseg == 0) return GK_OK;
        int rc = tables(T, C, nseg);
        if (rc != GK_OK) return rc;
        uint32_t *t_start, *t_count, *s_cfirst, *s_nchunks, *s_st;
        GK_TRY_HIP(c, scratch(c, "t_start", T, &t_start));
        GK_TRY_HIP(c, scratch(c, "t_count", T, &t_count));
        GK_TRY_HIP(c, scratch(c, "s_cfirst", nseg, &s_cfirst));
        GK_TRY_HIP(c, scratch(c, "s_nchunks", nseg, &s_nchunks));
        GK_TRY_HIP(c, scratch(c, "s_pstart", nseg, &s_st));
        GK_TRY_HIP(c, hipMemcpyAsync(t_start, ts.data(), 4 * T, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(t_count, tc.data(), 4 * T, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(c_first, cf.data(), 4 * C, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(c_ntiles, cn.data(), 4 * C, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(s_cfirst, scf.data(), 4 * nseg, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(s_nchunks, snc.data(), 4 * nseg, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipMemcpyAsync(s_st, sst.data(), 4 * nseg, hipMemcpyHostToDevice, c->stream));
        uint64_t *s_pref;
        GK_TRY_HIP(c, scratch(c, "s_ppref", nseg, &s_pref));
        GK_TRY_HIP(c, hipMemcpyAsync(s_pref, spf.data(), 8 * nseg, hipMemcpyHostToDevice, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        big_elems = n;
        // the reads() rule applied here, where the elements are held as pieces and not as a list of
        // buckets (pieces come as key/start forms or, from the prefetched L0, PackedL0): level_pass
        // below then chooses the same output format and finds an input it reads
        if (!reads(cur_fmt, level_format(level, hi, n, nseg))) {
            if (int rd = p88_detach()) return rd;
            uint64_t *pdev;
            GK_TRY_HIP(c, scratch(c, "p88_pieces", 3 * np, &pdev));
            std::vector<uint64_t> hp(3 * (uint64_t)np);
            for (uint32_t j = 0; j < np; ++j) {
                hp[j] = poff[j];
                hp[np + j] = plen[j];
                hp[2 * (uint64_t)np + j] = pbucket[j];
            }
            GK_TRY_HIP(c, hipMemcpyAsync(pdev, hp.data(), 8 * hp.size(), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(expand_p88_pieces_kernel, dim3(np, bucket_split(np)), dim3(256), 0, c->stream, pdev,
                               np, hi, B, p88_shi, const_cast<uint64_t *>(kin), lo16_l0, nd_l0,
                               const_cast<uint32_t *>(vin));
            GK_TRY_HIP(c, hipGetLastError());
            GK_TRY_HIP(c, hipStreamSynchronize(c->stream));  // (hp is released at return)
            cur_fmt = Fmt::KeyStartDigit;
        }
        rc = level_pass(level, hi, t_start, t_count, T, C, s_cfirst, s_nchunks, s_st, nseg, kin, vin, 0);
        if (rc != GK_OK) return rc;
        cur_big = 0;
        uint64_t before[kLocal];
        for (int k = 0; k < kLocal; ++k) before[k] = nloc[k];
        rc = classify(nseg << width(level), hi + width(level), 0, cur_big, nullptr, nullptr, 1, s_pref, width(level),
                      cur_fmt == Fmt::Compact ? 1 : 0);
        // (as levels(): a packed-pair level's local sub-buckets back to (key, start))
        if (rc == GK_OK && cur_fmt == Fmt::Pairs) rc = expand_pair_locals(before, 0);
        return rc == GK_OK ? expand_big(0) : rc;
    }

    unsigned tie_tiles() const { return (unsigned)std::max<uint64_t>((n + kTieTile - 1) / kTieTile, 1); }

    // The groups of >= 2 elements among the n that `flags` marks (a 1 starts a group), as *ng
    // (start, length) entries in scratch "tie_start" / "tie_len": the groups' firsts and lasts are
    // counted per tile, scanned, stored, and the lasts turned into lengths.  With no group (*ng = 0)
    // nothing is allocated or stored: the store pass would write nothing.  *tile_cnt / *tile_off
    // (optional): two of the pass's per-tile arrays (tie_tiles() + 1 words each), free for reuse.
    int tie_groups(const uint8_t *flags, uint32_t **g_start, uint32_t **g_len, uint64_t *ng,
                   uint32_t **tile_cnt = nullptr, uint32_t **tile_off = nullptr) {
        const unsigned ttiles = tie_tiles();
        uint32_t *cf, *cl, *of, *ol;
        GK_TRY_HIP(c, scratch(c, "tie_cnt_f", ttiles + 1, &cf));
        GK_TRY_HIP(c, scratch(c, "tie_cnt_l", ttiles + 1, &cl));
        GK_TRY_HIP(c, scratch(c, "tie_off_f", ttiles + 1, &of));
        GK_TRY_HIP(c, scratch(c, "tie_off_l", ttiles + 1, &ol));
        if (tile_cnt) *tile_cnt = cf;
        if (tile_off) *tile_off = of;
        hipLaunchKernelGGL(tie_bounds_kernel<false>, dim3(ttiles), dim3(256), 0, c->stream, flags, n, cf, cl, nullptr,
                           nullptr, nullptr, nullptr);
        GK_TRY_HIP(c, hipGetLastError());
        uint64_t ng2 = 0;
        GK_TRY_HIP(c, scan_u32_exclusive_pair(c, cf, of, cl, ol, ttiles, ng, &ng2));
        if (*ng != ng2) return fail(c, GK_E_HIP, "msd: tie group bounds do not pair up");
        if (*ng == 0) return GK_OK;
        GK_TRY_HIP(c, scratch(c, "tie_start", *ng + 64, g_start));
        GK_TRY_HIP(c, scratch(c, "tie_len", *ng + 64, g_len));
        hipLaunchKernelGGL(tie_bounds_kernel<true>, dim3(ttiles), dim3(256), 0, c->stream, flags, n, nullptr, nullptr,
                           of, ol, *g_start, *g_len);
        GK_TRY_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(tie_run_lengths_kernel, dim3((unsigned)std::min<uint64_t>((*ng + 255) / 256, 8192)),
                           dim3(256), 0, c->stream, *g_start, *g_len, *ng);
        GK_TRY_HIP(c, hipGetLastError());
        return GK_OK;
    }

    // the tie groups of keys[0] / vals[0], each sorted stably by the B-bit keys, in place: the groups
    // are the first buckets; global levels from level 1 with no bits sorted, local rounds, done copies
    int sort_tied(const uint32_t *g_start, const uint32_t *g_len, uint64_t ng) {
        cur_fmt = Fmt::KeyStart;
        int rc = classify(ng, 0, 0, cur_big, g_start, g_len, 2);
        if (rc != GK_OK) return rc;
        rc = levels(1, 0, 0);
        if (rc != GK_OK) return rc;
        return finish();
    }

    // Multi-word keys, phase > 0: the head flags of the order so far (buffer 0) mark the groups of
    // equal earlier words; sort each group of >= 2 by the key word of symbols [sym0, sym0 + nsym).
    int next_phase(int sym0, int nsym) {
        uint32_t *g_start, *g_len;
        uint64_t ng = 0;
        timer_begin(c, "msd_tie_groups", &slot);
        uint32_t *cf, *of;  // (per-tile counts and offsets: the member list below reuses them)
        if (int rc = tie_groups(heads, &g_start, &g_len, &ng, &cf, &of)) return rc;
        timer_end(c, slot);
        if (ng == 0) return GK_OK;
        const unsigned ttiles = tie_tiles();
        timer_begin(c, "msd_tie_encode", &slot);
        const unsigned grid = (unsigned)std::min<uint64_t>((ng + 3) / 4, (uint64_t)cus * 16);
        bool flat = ng > 4096;
        if (!flat) {  // few groups: flat too if they are large (one wave per group would be serial)
            std::vector<uint32_t> lens(ng);
            GK_TRY_HIP(c, hipMemcpyAsync(lens.data(), g_len, 4 * ng, hipMemcpyDeviceToHost, c->stream));
            GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
            uint64_t tot = 0;
            for (uint32_t v : lens) tot += v;
            flat = tot > (1u << 20);
        }
        if (flat) {  // many groups: the members listed from the head flags, then one thread per member
            // the list lives in the free key buffer (8 B per element; classify and the levels below
            // reuse it only after the encode has read the list)
            uint32_t *mlist = reinterpret_cast<uint32_t *>(c->keys[1]);
            hipLaunchKernelGGL(tie_members_kernel<false>, dim3(ttiles), dim3(256), 0, c->stream, heads, n, cf, nullptr,
                               nullptr);
            GK_TRY_HIP(c, hipGetLastError());
            uint64_t nm = 0;
            GK_TRY_HIP(c, scan_u32_exclusive_pub(c, cf, ttiles, of, &nm));
            hipLaunchKernelGGL(tie_members_kernel<true>, dim3(ttiles), dim3(256), 0, c->stream, heads, n, nullptr, of,
                               mlist);
            GK_TRY_HIP(c, hipGetLastError());
            const unsigned eg = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nm + 255) / 256, (uint64_t)cus * 16));
            if (ks.bits == 2)
                hipLaunchKernelGGL(tie_encode_list_kernel<2>, dim3(eg), dim3(256), 0, c->stream, c->sba, mlist, (uint32_t)nm,
                                   c->vals[0], c->keys[0], sym0, nsym, ks.symbols, ks.canonical);
            else
                hipLaunchKernelGGL(tie_encode_list_kernel<4>, dim3(eg), dim3(256), 0, c->stream, c->sba, mlist, (uint32_t)nm,
                                   c->vals[0], c->keys[0], sym0, nsym, ks.symbols, ks.canonical);
        } else if (ks.bits == 2)
            hipLaunchKernelGGL(tie_encode_kernel<2>, dim3(grid), dim3(256), 0, c->stream, c->sba, g_start, g_len,
                               (uint32_t)ng, c->vals[0], c->keys[0], sym0, nsym, ks.symbols, ks.canonical);
        else
            hipLaunchKernelGGL(tie_encode_kernel<4>, dim3(grid), dim3(256), 0, c->stream, c->sba, g_start, g_len,
                               (uint32_t)ng, c->vals[0], c->keys[0], sym0, nsym, ks.symbols, ks.canonical);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        B = ks.bits * nsym;
        ++phase;
        GK_TRY_HIP(c, hipMemsetAsync(ctr, 0, 4 * kCtrN, c->stream));
        ndone = 0;
        nbig = 0;
        for (int k = 0; k < kLocal; ++k) nloc[k] = loc_elems[k] = 0;
        return sort_tied(g_start, g_len, ng);
    }

    // Prefix doubling (gkm_doubling.hip rounds_by_groups): every run of >= 2 elements of keys[0] / vals[0]
    // that `flags` marks as one group (a 1 starts a group) sorted stably by the bkey-bit keys, in
    // place; the members' group heads in c->heads.  Elements outside those groups stay where they
    // are, so a round costs in proportion to the elements still tied, not to n.
    int sort_groups(const uint8_t *flags, int bkey) {
        uint32_t *g_start, *g_len;
        uint64_t ng = 0;
        if (int rc = tie_groups(flags, &g_start, &g_len, &ng)) return rc;  // (untimed: msd_groups covers the round)
        if (ng == 0) return GK_OK;
        B = bkey;
        phase = 1;  // (no compact or packed-pair levels: later-phase rules)
        return sort_tied(g_start, g_len, ng);
    }

    // global levels while the next-level list is non-empty; `in` holds the current buffer, hi
    // key bits are sorted
    // (cur_fmt carries over: a first level from pieces may have written packed pairs)
    int levels(int level, int hi, int in) {
        while (nbig > 0) {
            const int out = in ^ 1;
            uint32_t *ntl, *nch, *tfirst, *cfirst;
            GK_TRY_HIP(c, scratch(c, "s_ntiles", nbig, &ntl));
            GK_TRY_HIP(c, scratch(c, "s_nchunks", nbig, &nch));
            GK_TRY_HIP(c, scratch(c, "s_tfirst", nbig, &tfirst));
            GK_TRY_HIP(c, scratch(c, "s_cfirst", nbig, &cfirst));
            // the tile / chunk totals came with the list counters (classify, route_uniform)
            const uint64_t T = hs[kSumTiles], C = hs[kSumChunks];
            if (nbig <= kSegScanMax && !opt("GKM_TEST_SEG_SCAN_MULTI")) {
                hipLaunchKernelGGL(seg_tiles_scan_kernel, dim3(1), dim3(1024), 0, c->stream, big_len[cur_big], nbig,
                                   (uint32_t)kPTile, ctiles, tfirst, cfirst, nch);
                GK_TRY_HIP(c, hipGetLastError());
            } else {
                hipLaunchKernelGGL(seg_counts_kernel, dim3(grid256_min1(nbig)), dim3(256), 0, c->stream, big_len[cur_big],
                                   nbig, (uint32_t)kPTile, ctiles, ntl, nch);
                GK_TRY_HIP(c, hipGetLastError());
                GK_TRY_HIP(c, scan_u32_exclusive_pair_launch(c, ntl, tfirst, nch, cfirst, nbig));
            }
            if (opt("GKM_TEST_CHECK_TILES")) {  // (tests: the totals against the scans' own)
                uint32_t last[4];
                GK_TRY_HIP(c, hipMemcpyAsync(&last[0], tfirst + nbig - 1, 4, hipMemcpyDeviceToHost, c->stream));
                GK_TRY_HIP(c, hipMemcpyAsync(&last[1], cfirst + nbig - 1, 4, hipMemcpyDeviceToHost, c->stream));
                GK_TRY_HIP(c, hipMemcpyAsync(&last[2], nch + nbig - 1, 4, hipMemcpyDeviceToHost, c->stream));
                GK_TRY_HIP(c, hipMemcpyAsync(&last[3], big_len[cur_big] + nbig - 1, 4, hipMemcpyDeviceToHost, c->stream));
                GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
                if (last[0] + tiles_of(last[3], (uint32_t)kPTile) != T || last[1] + last[2] != C)
                    return fail(c, GK_E_HIP, "msd: level tile totals disagree with the bucket scan");
            }
            uint32_t *t_start, *t_count;
            GK_TRY_HIP(c, scratch(c, "t_start", T, &t_start));
            GK_TRY_HIP(c, scratch(c, "t_count", T, &t_count));
            int rc = tables(T, C, nbig);
            if (rc != GK_OK) return rc;
            hipLaunchKernelGGL(tile_table_kernel, dim3((unsigned)std::max<uint64_t>((std::max(T, C) + 255) / 256, 1)), dim3(256), 0,
                               c->stream, big_start[cur_big], big_len[cur_big], tfirst, cfirst, nbig,
                               (uint32_t)kPTile, (uint32_t)T, (uint32_t)C, ctiles, t_start, t_count, c_first, c_ntiles);
            const uint64_t in_big = big_elems;
            rc = level_pass(level, hi, t_start, t_count, T, C, cfirst, nch, big_start[cur_big], nbig, c->keys[in],
                            c->vals[in], out);
            if (rc != GK_OK) return rc;
            cur_big ^= 1;
            const bool pairs_out = cur_fmt == Fmt::Pairs;
            uint64_t before[kLocal];
            for (int k = 0; k < kLocal; ++k) before[k] = nloc[k];
            const uint64_t nsub = (uint64_t)nbig << width(level);
            // the level's input already small: its output's uniform buckets are dropped behind
            // the classify with one read-back for both (few_big_elems on the input's size)
            const bool fuse = !pairs_out && few_big_elems(level, in_big) && !opt("GKM_NO_FUSED_UNIFORM");
            rc = classify(nsub, hi + width(level), out, cur_big, nullptr, nullptr, 1, big_pref[cur_big ^ 1],
                          width(level), cur_fmt == Fmt::Compact ? 1 : 0, !fuse);
            if (fuse) {
                const uint64_t bound = std::min<uint64_t>(nsub, in_big / ((uint64_t)kBlockMax + 1));
                if (rc == GK_OK) rc = bound ? route_uniform(out, (uint32_t)bound, true) : classify_counts();
            } else {
                if (rc == GK_OK && pairs_out) rc = expand_pair_locals(before, out);
                if (rc == GK_OK) rc = expand_big(out);
                // (pairs: keys not comparable)
                if (rc == GK_OK && !pairs_out && nbig > 0 && few_big_elems(level, big_elems))
                    rc = route_uniform(out, nbig, false);
            }
            if (rc != GK_OK) return rc;
            ++level;
            hi += width(level - 1);
            in = out;
        }
        return GK_OK;
    }

    // one local class's kernel over a list of cnt buckets
    void local_launch(int k, uint32_t cnt, const uint2 *lst, uint64_t *k0, uint32_t *v0, const uint64_t *k1,
                      const uint32_t *v1, const Lists &nl, const Lists *d_nl, int round) {
        // common-prefix skip: re-listed buckets, later phases (repeats) and the block class; not
        // the first wave round of phase 0, where random keys differ right below the sorted bits
        const int skip = (round > 0 || phase > 0 || k == 3) ? 1 : 0;
        const uint32_t small = (round > 0 || phase > 0) ? kSmallLate : kSmall;
        // round 0 reads classify's entries, some of which may hold compact elements
        const CompactIn ci{round == 0 ? loc_pref[k] : nullptr, nd};
        // persistent grids of the workgroups that fit at once (occupancy API, per kernel)
        auto grid = [&](const void *fn, int threads) {
            uint64_t g = resident_grid(fn, threads, cnt);
            if (g >= 8) g &= ~7ull;  // the wave kernels' XCD-aware walk
            return dim3((unsigned)g);
        };
        // wave classes: msd_wave_kernel<I, waves per SIMD, keys written>
        auto wave = [&](auto fn_wk, auto fn_nk) {
            const void *fn = wkeys ? (const void *)fn_wk : (const void *)fn_nk;
            if (wkeys)
                hipLaunchKernelGGL(fn_wk, grid(fn, 64), dim3(64), 0, c->stream, lst, cnt, B, k0, v0, k1, v1, heads,
                                   d_nl, ctr, skip, small, ci.pref, ci.nd);
            else
                hipLaunchKernelGGL(fn_nk, grid(fn, 64), dim3(64), 0, c->stream, lst, cnt, B, k0, v0, k1, v1, heads,
                                   d_nl, ctr, skip, small, ci.pref, ci.nd);
        };
        switch (k) {
        case 0:
            wave(msd_wave_kernel<4, kWaveOcc4, true, kWaveR4>, msd_wave_kernel<4, kWaveOcc4, false, kWaveR4>);
            break;
        case 1:
            wave(msd_wave_kernel<8, kWaveOcc8, true, kWaveR8>, msd_wave_kernel<8, kWaveOcc8, false, kWaveR8>);
            break;
        case 2:
            wave(msd_wave_kernel<16, kWaveOcc16, true, kWaveR16>, msd_wave_kernel<16, kWaveOcc16, false, kWaveR16>);
            break;
        case 3:
            hipLaunchKernelGGL((msd_local_kernel<kBT, kBI, kBR>),
                               grid((const void *)msd_local_kernel<kBT, kBI, kBR>, kBT), dim3(kBT), 0, c->stream, lst,
                               cnt, B, k0, v0, k1, v1, heads, nl, ctr, skip,
                               (uint32_t)kSmall, wkeys, ci);  // the block class keeps kSmall: 96 measured slower (A/B)
            break;
        case 5:
            hipLaunchKernelGGL((msd_local_kernel<kBT2, kBI, kBR2>),
                               grid((const void *)msd_local_kernel<kBT2, kBI, kBR2>, kBT2), dim3(kBT2), 0, c->stream,
                               lst, cnt, B, k0, v0, k1, v1, heads, nl, ctr, skip, (uint32_t)kSmall, wkeys, ci);
            break;
        default:
            hipLaunchKernelGGL(msd_tiny_kernel, dim3((cnt + 255) / 256), dim3(256), 0, c->stream, lst, cnt, k0, v0, k1,
                               v1, heads, wkeys, ci, B);
        }
    }

    // local rounds (generation g lists -> re-listed sub-buckets in generation g ^ 1), done copies.
    int finish() {
        const uint64_t max_spill = n / (kSmall + 1) + 1024;
        uint64_t pending = 0;
        for (int k = 0; k < kLocal; ++k) {
            GK_TRY_HIP(c, grow_keep(c, kLocName[k][0], std::max<uint64_t>(nloc[k], max_spill), nloc[k], &loc[k][0]));
            GK_TRY_HIP(c, grow_keep(c, kLocName[k][1], max_spill, 0, &loc[k][1]));
            pending += nloc[k];
        }
        if (int rc = grow_done(max_spill)) return rc;
        int g = 0, round = 0;
        while (pending > 0) {
            const int ng = g ^ 1;
            // the re-list counters of this round start from 0 (the done count carries on)
            GK_TRY_HIP(c, hipMemsetAsync(ctr + kCtrLoc, 0, 4 * kLocal, c->stream));
            const Lists nl = lists(ng, 0);
            Lists *d_nl = nullptr;
            GK_TRY_HIP(c, scratch(c, "lists_dev", 1, &d_nl));
            hipLaunchKernelGGL(lists_store_kernel, dim3(1), dim3(1), 0, c->stream, nl, d_nl);
            GK_TRY_HIP(c, hipGetLastError());
            for (int k = 0; k < kLocal; ++k) {
                if (!nloc[k]) continue;
                timer_begin(c, round == 0 ? kLocTimer[k][0] : kLocTimer[k][1], &slot);
                if (round == 0) timer_units(c, slot, loc_elems[k]);
                const uint32_t cnt = (uint32_t)nloc[k];
                uint64_t *k0 = c->keys[0], *k1 = c->keys[1];
                uint32_t *v0 = c->vals[0], *v1 = c->vals[1];
                const uint2 *lst = loc[k][g];
                const bool trace = opt("GKM_MSD_TRACE") != nullptr;  // (read per launch: a few per sort)
                hipEvent_t t0 = nullptr, t1 = nullptr;
                if (trace) {
                    hipEventCreate(&t0);
                    hipEventCreate(&t1);
                    hipEventRecord(t0, c->stream);
                }
                local_launch(k, cnt, lst, k0, v0, k1, v1, nl, d_nl, round);
                GK_TRY_HIP(c, hipGetLastError());
                timer_end(c, slot);
                if (trace) {  // diagnostics: one line per local launch
                    hipEventRecord(t1, c->stream);
                    hipEventSynchronize(t1);
                    float ms = 0;
                    hipEventElapsedTime(&ms, t0, t1);
                    std::fprintf(stderr, "[msd] phase %d round %d class %d buckets %u: %.3f ms\n", phase, round, k,
                                 cnt, ms);
                    hipEventDestroy(t0);
                    hipEventDestroy(t1);
                }
            }
            int rc = read_ctr();
            if (rc != GK_OK) return rc;
            pending = 0;
            for (int k = 0; k < kLocal; ++k) {
                nloc[k] = h[kCtrLoc + k];
                pending += nloc[k];
            }
            ndone = h[kCtrDone];
            g = ng;
            if (++round > 64) return fail(c, GK_E_HIP, "msd local rounds did not converge");
        }
        if (ndone > 0) {
            hipLaunchKernelGGL(done_copy_kernel, dim3((unsigned)ndone, bucket_split(ndone)), dim3(256), 0, c->stream,
                               dn_start, dn_len,
                               dn_par, c->vals[1], c->vals[0], wkeys ? c->keys[1] : nullptr, c->keys[0], heads);
            GK_TRY_HIP(c, hipGetLastError());
        }
        c->heads = heads;
        c->heads_valid = true;
        c->cur = 0;
        return GK_OK;
    }

    // The tail of a sort entry point, behind its first partition: the remaining global levels (from
    // `level`, hi key bits sorted, buffer `in` current), the local rounds and done copies, the later
    // phases of multi-word keys; then the total timer ends.  An error stops the work there.
    // rc: the first partition's result -- entry points that used to end the total timer behind a failed
    // first partition pass it on, the others return before; open_on_level_error: msd_sort and
    // msd_shard_sort return from a failed global level at once, with the timer open (kept as it was).
    int run_from(int rc, int level, int hi, int in, bool open_on_level_error = false) {
        if (rc == GK_OK) {
            rc = levels(level, hi, in);
            if (rc != GK_OK && open_on_level_error) return rc;
        }
        if (rc == GK_OK) rc = finish();
        const int spw = symbols_per_word();
        for (int ph = 1; ph < phases() && rc == GK_OK; ++ph)
            rc = next_phase(ph * spw, std::min(spw, ks.symbols - ph * spw));
        timer_end(c, total_slot);
        return rc;
    }

    // key-range shards: the ownership-digit histogram of the byte sequence, 2- or 4-bit keys
    template <int BITS, bool CANON>
    void hist_launch(const L0Args &a, uint32_t ntiles, uint32_t *gh) {
        hipLaunchKernelGGL((own_hist_kernel<BITS, CANON>),
                           dim3(resident_grid((const void *)own_hist_kernel<BITS, CANON>, kST, ntiles)), dim3(kST), 0,
                           c->stream, a, ntiles, gh);
    }

    // key-range shards: the single-pass select over the byte sequence -- chunks of *tpw tiles per
    // workgroup, one region of *tpw * kSTile elements each in keys[1] / vals[1] (room for every
    // position: no count pass), the chunks' counts in wave_cnt.  Persistent grid = the workgroups that
    // fit at once (a second round of workgroups would start only when the first ones have walked
    // all their tiles)
    template <int BITS, bool CANON>
    void select_launch(const L0Args &a, Dig d0, uint32_t ntiles, uint32_t *wave_cnt, uint32_t *tpw, uint32_t *nchunk) {
        const unsigned sgrid = resident_grid((const void *)msd0_select_kernel<BITS, CANON>, kST, ntiles);
        *tpw = (ntiles + sgrid - 1) / sgrid;
        *nchunk = (ntiles + *tpw - 1) / *tpw;
        hipLaunchKernelGGL((msd0_select_kernel<BITS, CANON>), dim3(*nchunk), dim3(kST), 0, c->stream, a, d0, ntiles,
                           *tpw, wave_cnt, c->keys[1], c->vals[1], nd);
    }

    // key-range shards: the select's pieces.  Region w of keys[1] / vals[1] starts at w * stride and
    // holds cnt[w] kept k-mers (cnt on the device, nreg regions); the non-empty ones, in position
    // order, are the pieces of the first level.  *found: their sum, the stage's units.
    int harvest_pieces(const uint32_t *cnt, uint64_t nreg, uint64_t stride, int select_slot, std::vector<uint64_t> *poff,
                       std::vector<uint64_t> *plen, uint64_t *found) {
        std::vector<uint32_t> kc(nreg);
        GK_TRY_HIP(c, hipMemcpyAsync(kc.data(), cnt, 4 * nreg, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        for (uint64_t w = 0; w < nreg; ++w) {
            if (!kc[w]) continue;
            poff->push_back(w * stride);
            plen->push_back(kc[w]);
            *found += kc[w];
        }
        timer_units(c, select_slot, *found);  // (stage rates: kept k-mers out, the whole sequence in)
        if (*found > 0xFFFFFFFFull) return fail(c, GK_E_ARG, "more k-mers than uint32 start indices can address");
        return GK_OK;
    }
};

// The enumerated k-mers of the whole sequence (gk_sort's fixed-length path, k <= 64), in one-word
// phases (MsdDriver::phases).
int msd_sort(gk_ctx *c, const KeySpec &ks, uint64_t n, bool acgt_keys, bool *keys_final) {
    MsdDriver d(c, ks);
    d.acgt_keys = acgt_keys;
    int rc = d.begin(n, keys_final);
    if (rc != GK_OK) return rc;
    if (d.phases() == 1) d.enable_wide_l0();
    // canonical 2-bit keys with a full 64-bit first word (k >= 32; C5): an 8-bit L0 leaves 48 bits
    // behind the next level -- packed pairs there and a compact level after them, which the 7-bit
    // L0's 49 and 41 bits do not allow (C5 219-221 -> 216.7-216.9 ms, profiles/r4/l08_ab.txt; the
    // same change made C4, 62-bit keys, 5 ms slower)
    if (ks.bits == 2 && ks.canonical && d.B == 64 && !opt("GKM_LEVEL_BITS")) d.wsched[0] = 8;
    d.use_resident_pack();
    uint64_t found = 0;
    rc = d.l0_count(0, c->sba_len, 0, 0xFFFFFFFFu, &found);  // all digits owned
    if (rc != GK_OK) return rc;
    if (found != n) return fail(c, GK_E_HIP, "msd: k-mer count differs from the enumeration");
    int in = 0;
    rc = d.l0_start(found, &in);
    if (rc != GK_OK) return rc;
    return d.run_from(GK_OK, 1, d.width(0), in, true);
}

// ---------------------------------------------------------------------------------------------
// Prefetched L0 (gk_sort_hint).  The end-to-end interval of a sort -- the sequence in host memory
// to the sorted product in HBM -- is the packed transfer (host-bound: ~20 ms for 3.1 Gb) followed
// by the sort, whose first pass (L0 count + partition, ~14 ms at C3) needs only the sequence.  With
// a hint, gk_set_sequence runs that pass while the sequence streams in: the k-mer starts [0, n) of
// an ACGT sba (any number of contigs: the '$' separators are stops of the L0 pass, round 6) are cut
// into regions of whole L0 tiles of positions; as soon as the transfer has
// unpacked a region's bytes (and its last tile's halo) on the context's stream, the region is
// counted, scanned and partitioned on the prefetch stream into keys[1] / vals[1] / the digit bytes
// at output indices from its first position (MsdDriver::l0_region), and its 2^w0 buckets become
// pieces.  gk_sort(k) then starts at the first level from those pieces (msd_sort_prefetched, the
// key-range shards' first_level_from_pieces) -- the same stable order: a bucket's pieces are taken
// in region order, i.e. start order.  Any other use of the buffers drops the prefetch (pre_drop).
// ---------------------------------------------------------------------------------------------
struct L0Prefetch {
    KeySpec ks{};
    uint64_t len = 0, n = 0;        // sba bytes, k-mer starts
    uint32_t nreg = 0, tpr = 0;     // regions, L0 tiles of the largest region
    uint32_t nc_max = 0, next = 0;  // chunk-table entries per region; next region to launch
    int w0 = 7, w1 = 8;
    bool p88 = false;               // the packed L0 output (MsdDriver::p88_wanted for n)
    int p88_shi = 0;
    uint32_t *tab = nullptr;        // per region: c_first[nc_max], c_ntiles[nc_max], misc[4]
    uint32_t *pieces = nullptr;     // per region: 2^w0 bases, then 2^w0 counts
    std::vector<uint64_t> first;    // first L0 tile of each region (+ the end)
    uint64_t lo(uint32_t r) const { return first[r] * kP0Tile; }
    uint64_t hi(uint32_t r) const { return std::min<uint64_t>(first[r + 1] * kP0Tile, n); }
    uint32_t tiles(uint32_t r) const { return (uint32_t)((hi(r) - lo(r) + kP0Tile - 1) / kP0Tile); }
    // bytes a region's tiles read: each tile loads its positions plus a 96-byte halo
    uint64_t need(uint32_t r) const { return std::min<uint64_t>(lo(r) + (uint64_t)tiles(r) * kP0Tile + 128, len); }
};

static KeySpec hint_spec(uint32_t k) {
    KeySpec ks{};
    ks.bits = 2;
    ks.symbols = (int)k;
    ks.min_len = (int)k;
    ks.words = 1;
    ks.total_bits = 2 * (int)k;
    return ks;
}

bool prefetch_matches(const gk_ctx *c, const KeySpec &ks, uint64_t n) {
    return c->pre_valid && c->enumerated && ks.bits == 2 && ks.symbols == (int)c->pre_k &&
           ks.min_len == ks.symbols && ks.words == 1 && ks.lenbits == 0 && !ks.canonical &&
           n + ks.symbols - 1 <= c->sba_len;  // (acgt_only: the class A of a mixed sba, gkm_split.hip)
}

int prefetch_plan(gk_ctx *c, uint64_t len, L0Prefetch **out) {
    *out = nullptr;
    const uint32_t k = c->hint_k;
    if (k < 8 || k > 32 || len < (uint64_t)k + kP0Tile) return GK_OK;
    const KeySpec ks = hint_spec(k);
    MsdDriver d(c, ks);
    if (d.width(0) != 7 && d.width(0) != kGR) return GK_OK;  // (the wide L0 has its own tiles)
    auto *p = new L0Prefetch();
    p->ks = ks;
    p->len = len;
    p->n = len - k + 1;
    p->w0 = d.width(0);
    p->w1 = d.width(1);
    d.allow_c79 = true;
    d.n = p->n;
    p->p88 = d.p88_wanted();
    p->p88_shi = 64 - (d.B - p->w0 - 8);
    const uint64_t nt = (p->n + kP0Tile - 1) / kP0Tile;
    // regions: GKM_PREFETCH_REGIONS (default 16); the last region's pass is what the transfer
    // cannot hide
    const char *e = opt("GKM_PREFETCH_REGIONS");
    const uint64_t want = std::max<uint64_t>(1, e && *e ? std::strtoull(e, nullptr, 10) : 16);
    // equal regions, but the last one's share is cut into halving pieces (1/2, 1/4, 1/8, 1/8 of it):
    // the pass of the last region to land is what the transfer cannot hide
    const uint64_t tpr = std::max<uint64_t>(1, (nt + want - 1) / want);
    for (uint64_t f = 0; f < nt; f += tpr) {
        const uint64_t e = std::min(nt, f + tpr);
        if (e == nt && e - f >= 8) {
            const uint64_t m = e - f;
            for (uint64_t g : {f, f + m / 2, f + 3 * m / 4}) p->first.push_back(g);
            p->first.push_back(f + 7 * m / 8);
        } else {
            p->first.push_back(f);
        }
    }
    p->first.push_back(nt);
    p->nreg = (uint32_t)(p->first.size() - 1);
    p->tpr = (uint32_t)tpr;
    p->nc_max = (p->tpr + d.ctiles - 1) / d.ctiles;
    const uint32_t R = 1u << p->w0, stride = 2 * p->nc_max + 4;
    int rc = ensure_elems(c, len, 1);  // keys[1] / vals[1] by position (n <= len)
    if (rc != GK_OK) {
        delete p;
        return rc;
    }
    GK_TRY_HIP(c, msd_tables());
    uint8_t *ndp;
    uint32_t *dummy;
    if (!p->p88) GK_TRY_HIP(c, scratch(c, "msd_nd", len + 64, &ndp));  // (packed: in vals[1], MsdDriver::p88_place)
    GK_TRY_HIP(c, scratch(c, "pre_tables", (uint64_t)p->nreg * stride, &p->tab));
    GK_TRY_HIP(c, scratch(c, "pre_pieces", (uint64_t)p->nreg * 2 * R, &p->pieces));
    GK_TRY_HIP(c, scratch(c, "s_misc", 4, &dummy));
    rc = d.tables(p->tpr, p->nc_max, 1);
    if (rc != GK_OK) {
        delete p;
        return rc;
    }
    std::vector<uint32_t> h((uint64_t)p->nreg * stride, 0);
    for (uint32_t r = 0; r < p->nreg; ++r) {
        uint32_t *t = h.data() + (uint64_t)r * stride;
        const uint32_t ntr = p->tiles(r), ncr = (ntr + d.ctiles - 1) / d.ctiles;
        for (uint32_t j = 0; j < ncr; ++j) {
            t[j] = j * d.ctiles;
            t[p->nc_max + j] = std::min<uint32_t>(d.ctiles, ntr - j * d.ctiles);
        }
        t[2 * p->nc_max] = 0;                        // s_cfirst
        t[2 * p->nc_max + 1] = ncr;                  // s_nchunks
        t[2 * p->nc_max + 2] = (uint32_t)p->lo(r);   // s_start: outputs by position
    }
    GK_TRY_HIP(c, hipMemcpy(p->tab, h.data(), 4 * h.size(), hipMemcpyHostToDevice));
    if (!c->pre_stream) GK_TRY_HIP(c, hipStreamCreateWithFlags(&c->pre_stream, hipStreamNonBlocking));
    if (!c->pre_done) GK_TRY_HIP(c, hipEventCreateWithFlags(&c->pre_done, hipEventDisableTiming));
    while (c->pre_ev.size() < p->nreg) {
        hipEvent_t ev;
        GK_TRY_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->pre_ev.push_back(ev);
    }
    *out = p;
    return GK_OK;
}

int prefetch_launch(gk_ctx *c, L0Prefetch *p, uint64_t landed) {
    if (!p || p->next >= p->nreg || landed < p->need(p->next)) return GK_OK;
    // every unpack enqueued so far (on the transfer's unpack stream); the regions now covered wait
    // for them
    GK_TRY_HIP(c, hipEventRecord(c->pre_ev[p->next], c->unpack_stream ? c->unpack_stream : c->stream));
    GK_TRY_HIP(c, hipStreamWaitEvent(c->pre_stream, c->pre_ev[p->next], 0));
    // the regions run on the prefetch stream; every return below restores the context's stream
    struct StreamSwap {
        gk_ctx *c;
        hipStream_t keep;
        ~StreamSwap() { c->stream = keep; }
    } swap{c, c->stream};
    c->stream = c->pre_stream;
    MsdDriver d(c, p->ks);
    if (p->p88) {  // the regions' low start bits and digit bytes in vals[1] (p88_place)
        d.p88_place(1);
        d.nd = d.nd_l0;
        d.p88 = true;
        d.p88_shi = p->p88_shi;
    } else {
        GK_TRY_HIP(c, scratch(c, "msd_nd", p->len + 64, &d.nd));
    }
    const uint32_t R = 1u << p->w0, stride = 2 * p->nc_max + 4;
    int rc = GK_OK;
    int slot;
    timer_begin(c, "prefetch_l0", &slot);
    uint64_t units = 0;
    for (; rc == GK_OK && p->next < p->nreg && landed >= p->need(p->next); ++p->next) {
        const uint32_t r = p->next, ntr = p->tiles(r);
        rc = d.l0_region(p->lo(r), p->hi(r), ntr, (ntr + d.ctiles - 1) / d.ctiles, p->nc_max,
                         p->tab + (uint64_t)r * stride, p->len + 16, p->pieces + (uint64_t)r * 2 * R);
        units += p->hi(r) - p->lo(r);
    }
    timer_units(c, slot, units);
    timer_end(c, slot);
    return rc;
}

int prefetch_finish(gk_ctx *c, L0Prefetch *p, bool ok) {
    if (!p) return GK_OK;
    int rc = GK_OK;
    if (ok) rc = prefetch_launch(c, p, p->len);
    if (p->next > 0) {  // later work on the context's stream comes after the prefetch's
        GK_TRY_HIP(c, hipEventRecord(c->pre_done, c->pre_stream));
        GK_TRY_HIP(c, hipStreamWaitEvent(c->stream, c->pre_done, 0));
    }
    c->pre_valid = ok && rc == GK_OK && p->next == p->nreg;
    c->pre_k = (uint32_t)p->ks.symbols;
    c->pre_regions = p->nreg;
    c->pre_w0 = p->w0;
    c->pre_w1 = p->w1;
    c->pre_p88_shi = p->p88 ? p->p88_shi : 0;
    delete p;
    return rc;
}

// gk_sort(k) after a prefetched L0: the regions' buckets are the pieces of the first level
int msd_sort_prefetched(gk_ctx *c, const KeySpec &ks, uint64_t n, bool acgt_keys, bool *keys_final) {
    c->pre_valid = false;  // consumed
    MsdDriver d(c, ks);
    if (d.width(0) != c->pre_w0 || d.width(1) != c->pre_w1)  // (widths changed)
        return msd_sort(c, ks, n, acgt_keys, keys_final);
    d.acgt_keys = acgt_keys;
    int rc = d.begin(n, keys_final, ks.total_bits);  // (one word: prefetch_matches)
    if (rc != GK_OK) return rc;
    const uint32_t R = 1u << c->pre_w0, nreg = c->pre_regions;
    uint32_t *pieces;
    GK_TRY_HIP(c, scratch(c, "pre_pieces", (uint64_t)nreg * 2 * R, &pieces));
    std::vector<uint32_t> h((uint64_t)nreg * 2 * R);
    GK_TRY_HIP(c, hipMemcpyAsync(h.data(), pieces, 4 * h.size(), hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> poff, plen;
    std::vector<uint32_t> pb;
    for (uint32_t b = 0; b < R; ++b)
        for (uint32_t r = 0; r < nreg; ++r) {  // a bucket's pieces in region order = start order
            const uint32_t cnt = h[(uint64_t)r * 2 * R + R + b];
            if (!cnt) continue;
            poff.push_back(h[(uint64_t)r * 2 * R + b]);
            plen.push_back(cnt);
            pb.push_back(b);
        }
    if (c->pre_p88_shi) {  // the regions wrote the packed L0 form (its side arrays in vals[1])
        d.p88_place(1);
        d.nd = d.nd_l0;
        d.cur_fmt = MsdDriver::Fmt::PackedL0;
        d.p88_shi = c->pre_p88_shi;
    } else {
        GK_TRY_HIP(c, scratch(c, "msd_nd", c->sba_len + 64, &d.nd));
        d.cur_fmt = MsdDriver::Fmt::KeyStartDigit;  // (either way the regions wrote the level-1 digit bytes)
    }
    rc = d.first_level_from_pieces(c->keys[1], c->vals[1], poff.data(), plen.data(), pb.data(),
                                   (uint32_t)poff.size(), 1, d.width(0));
    return d.run_from(rc, 2, d.width(0) + d.width(1), 0);
}

// multi-GPU send side: k-mers starting in [lo, hi) partitioned by their top kGR key bits
int msd_shard_partition(gk_ctx *c, const KeySpec &ks, uint64_t lo, uint64_t hi, uint64_t *kout, uint32_t *vout,
                        uint64_t cap, uint64_t *hist, uint64_t *count) {
    MsdDriver d(c, ks);
    d.B = ks.bits * std::min(ks.symbols, 64 / ks.bits);  // the first key word (see msd_sort)
    d.wsched[0] = kGR;  // the exchange splits by kGR-bit buckets (msd_radix_bits)
    GK_TRY_HIP(c, msd_tables());
    // (this test used to read "res_pk && acgt && bits == 2", without "|| ks.acgt_only": the same here,
    // where the key spec is gk_shard_partition's shard_spec -- acgt_only = 0, and 2-bit keys only
    // for an ACGT sba)
    d.use_resident_pack();
    int rc = d.l0_count(lo, hi, 0, 0xFFFFFFFFu, count);  // all digits owned
    if (rc == GK_OK) rc = d.l0_partition(kout, vout, cap, *count);
    if (rc != GK_OK) return rc;
    std::vector<uint32_t> hc(kGRadix);
    GK_TRY_HIP(c, hipMemcpyAsync(hc.data(), d.seg_cnt, 4 * kGRadix, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));  // the caller's exchange reads kout / vout next
    for (int i = 0; i < kGRadix; ++i) hist[i] = hc[i];
    return GK_OK;
}

// multi-GPU receive side: sort n received k-mers (buckets as pieces) into keys[0] / vals[0]
int msd_shard_sort(gk_ctx *c, const KeySpec &ks, const uint64_t *kin, const uint32_t *vin, const uint64_t *poff,
                   const uint64_t *plen, const uint32_t *pbucket, uint32_t np, bool *keys_final) {
    MsdDriver d(c, ks);
    d.wsched[0] = kGR;  // pieces are kGR-bit buckets
    int rc = d.begin(c->n, keys_final);
    if (rc != GK_OK) return rc;
    if (!kin) {
        // starts only (GK_SHARD_STARTS_ONLY): every received k-mer's key from the rank's own packed copy
        // of the sequence (a sender's piece holds ascending starts of one position range, so the
        // words read stay close), with the level-1 digit byte its count pass reads
        const uint64_t *pk = nullptr;
        const uint32_t *pd = nullptr;
        if (d.use_resident_pack()) {  // (starts-only shards: an ACGT sba, 2-bit keys -- shard_spec)
            pk = c->res_code;
        } else {
            int rp = pack_sequence(c, &pk, &pd);
            if (rp != GK_OK) return rp;
        }
        GK_TRY_HIP(c, scratch(c, "msd_nd", c->n + 64, &d.nd));
        int slot;
        timer_begin(c, "shard_keys", &slot);
        timer_units(c, slot, c->n);
        hipLaunchKernelGGL(keys_from_starts_kernel, dim3(grid256_cap64k(c->n)), dim3(256), 0, c->stream, pk, vin, c->n,
                           d.B, dig_at(d.B, kGR, d.width(1)), c->keys[1], d.nd);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        kin = c->keys[1];
        d.cur_fmt = MsdDriver::Fmt::KeyStartDigit;
    }
    rc = d.first_level_from_pieces(kin, vin, poff, plen, pbucket, np);
    if (rc != GK_OK) return rc;
    return d.run_from(GK_OK, 2, kGR + d.width(1), 0, true);
}

// One-word keys already in memory (keys[cur] / vals[cur], n = c->n; the low total_bits bits of
// each key significant), sorted stably by the MSD levels over the keys themselves -- 8-bit digits
// from the top, packed pairs and a compact level where the bits allow, the same finishing kernels --
// instead of one LSD pass per 8 bits: two global passes and the local rounds for 1e8 keys where
// the LSD sort made six.  Result in keys[0] / vals[0] (c->cur = 0), the keys final; radix_sort's
// contract otherwise (gkm_sort.hip).
int msd_sort_keys(gk_ctx *c, int total_bits) {
    KeySpec kk{};
    kk.bits = 8;  // (no sequence-derived L0: every level reads the keys, 8-bit digits)
    kk.symbols = (total_bits + 7) / 8;
    kk.min_len = 1;
    kk.words = 1;
    kk.total_bits = total_bits;
    MsdDriver d(c, kk);
    // digit widths: as few global levels as leave buckets of <= ~400 keys for the one-wave
    // finishing classes (1e8 keys: 6 + 6 + 6 bits, buckets of ~380), the bits spread evenly; two
    // 8-bit levels left 1.5 K-key buckets to the block-local class, which ran 3.6 ms for 1e8 keys
    if (!opt("GKM_LEVEL_BITS")) {
        int b = 0;
        while (b < total_bits && (c->n >> b) > 400) ++b;
        const int L = std::max(1, (b + 7) / 8);
        const int w = std::max(6, std::min(8, (b + L - 1) / L));
        for (int l = 0; l < kMaxLevels; ++l) d.wsched[l] = l < L ? w : kGR;
    }
    const int in = c->cur;
    int rc = d.begin(c->n, nullptr, total_bits);  // (one word of up to 8 "symbols": the keys end final in keys[0])
    if (rc != GK_OK) return rc;
    uint32_t *one;
    GK_TRY_HIP(c, scratch(c, "keys_bucket", 2, &one));
    const uint32_t hb[2] = {0, (uint32_t)c->n};
    GK_TRY_HIP(c, hipMemcpyAsync(one, hb, 8, hipMemcpyHostToDevice, c->stream));
    rc = d.classify(1, 0, in, 0, one, one + 1);  // all keys as one bucket, no bits sorted
    rc = d.run_from(rc, 0, 0, in);
    c->cur = 0;  // (whatever the outcome)
    return rc;
}

// sort_doubling's rounds: the tied groups of keys[0] / vals[0] (flags: 1 starts a group) sorted by
// their bkey-bit keys (MsdDriver::sort_groups)
int msd_sort_groups(gk_ctx *c, const uint8_t *flags, int bkey) {
    KeySpec kk{};
    kk.bits = 8;
    kk.symbols = (bkey + 7) / 8;
    kk.min_len = 1;
    kk.words = 1;
    kk.total_bits = bkey;
    MsdDriver d(c, kk);
    d.B = bkey;
    d.wkeys = 1;
    timer_begin(c, "msd_groups", &d.total_slot);
    int rc = d.init(c->n);
    if (rc == GK_OK) rc = d.sort_groups(flags, bkey);
    timer_end(c, d.total_slot);
    return rc;
}

int msd_radix_bits() { return kGR; }
hipError_t rank_mode_msd(int ballot) { return set_rank_ballot_here(ballot); }

// the key-range ranks fuse their select into the L0 when their digit share is >= 1 / this: the
// emulated C3 rank (tools/range_emulate.py, profiles/r5/emu_fused_ab.txt) ran 42.3 against 45.0 ms
// fused at N = 2, but 26.0 against 23.7 at N = 4 and 18.1 against 13.5 at N = 8 -- the L0 over the
// whole sequence costs ~7.7 ms even when it stores an eighth of it
constexpr uint64_t kFusedMaxRanks = 2;

// L0 digit width of the key-range shards: 7 bits for 2-bit keys (as msd_sort), 8 otherwise
static int range_width(const KeySpec &ks) { return ks.bits == 2 ? 7 : kGR; }

// Ownership digits of the key-range shards: the ranks' ranges are cut on the top 12 bits of 2-bit
// keys (k >= 6; 2k bits below), so a hot 7-bit L0 digit of a skewed genome is split between ranks;
// 4-bit keys keep 8 bits.  The first partition level after the select still uses range_width.
int range_own_bits(const KeySpec &ks) {
    const int B = ks.bits * std::min(ks.symbols, 64 / ks.bits);
    return ks.bits == 2 ? std::min(12, B) : std::min(kGR, B);
}

int msd_l0_histogram(gk_ctx *c, const KeySpec &ks, uint64_t lo, uint64_t hi, uint64_t *hist, int *bits) {
    MsdDriver d(c, ks);
    d.B = ks.bits * std::min(ks.symbols, 64 / ks.bits);  // the first key word (see msd_sort)
    GK_TRY_HIP(c, msd_tables());
    d.use_resident_pack();
    const int ob = range_own_bits(ks);
    L0Args a{c->sba, lo, std::max(hi, lo), ks.symbols, d.B, ks.acgt_only};
    a.own_bits = ob;
    a.pk_code = d.l0a.pk_code;
    a.pk_dol = d.l0a.pk_dol;
    uint32_t *gh;
    GK_TRY_HIP(c, scratch(c, "own_hist", 4096, &gh));
    GK_TRY_HIP(c, hipMemsetAsync(gh, 0, 4 * 4096, c->stream));
    const uint32_t ntiles = (uint32_t)std::max<uint64_t>((a.hi - lo + kSTile - 1) / kSTile, 1);
    int slot;
    timer_begin(c, "histogram", &slot);
    timer_units(c, slot, a.hi - lo);
    if (ks.bits == 2 && !ks.canonical && a.pk_code && ks.symbols <= 32 && a.hi > lo) {
        const uint64_t resident = (uint64_t)d.cus * resident_per_cu(c, (const void *)own_hist_rsel_kernel, kRselW * 64);
        const uint64_t G = (a.hi + 31) / 32 - lo / 32;
        const uint64_t gpb = std::max<uint64_t>((G + resident - 1) / resident, 1);
        hipLaunchKernelGGL(own_hist_rsel_kernel, dim3((unsigned)((G + gpb - 1) / gpb)), dim3(kRselW * 64), 0, c->stream,
                           a, gpb, gh);
    } else if (ks.bits == 2) {
        if (ks.canonical) d.hist_launch<2, true>(a, ntiles, gh);
        else d.hist_launch<2, false>(a, ntiles, gh);
    } else {
        if (ks.canonical) d.hist_launch<4, true>(a, ntiles, gh);
        else d.hist_launch<4, false>(a, ntiles, gh);
    }
    GK_TRY_HIP(c, hipGetLastError());
    timer_end(c, slot);
    std::vector<uint32_t> hc(1u << ob);
    GK_TRY_HIP(c, hipMemcpyAsync(hc.data(), gh, 4u << ob, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < (1 << ob); ++i) hist[i] = hc[i];
    *bits = ob;
    return GK_OK;
}

int msd_sort_range(gk_ctx *c, const KeySpec &ks, uint32_t digit_lo, uint32_t digit_hi, bool acgt_keys, uint64_t *n_kept,
                   bool *keys_final) {
    MsdDriver d(c, ks);
    d.acgt_keys = acgt_keys;
    d.wsched[0] = range_width(ks);
    // (packed-pair levels where the bits fit: the first level from the select's pieces has 55 bits
    // left at C3, its L1 writes the pairs)
    int rc = d.begin(MsdDriver::kInitLater, keys_final);  // (the lists once the select or the count has found n)
    if (rc != GK_OK) return rc;
    GK_TRY_HIP(c, msd_tables());
    const uint64_t L = c->sba_len;
    const int ob = range_own_bits(ks);
    const uint32_t span = digit_hi > digit_lo ? digit_hi - digit_lo : 0;
    d.use_resident_pack();  // (the select and the fused L0 both read it)
    c->n = 0;  // nothing in the buffers survives: ensure_elems copies none
    c->cur = 0;
    // Fused select (round 5): when the rank keeps a large share of the k-mers, its L0 count and
    // partition run over the whole sequence and keep only the owned k-mers (msd0_pipe_kernel<...,
    // OWN>), as msd_sort's L0 does for all of them -- no select pass, no 13-byte write and re-read
    // per kept k-mer, and the packed L0 output.  With a small share the whole-sequence L0 (count,
    // packing and ranking of every position) costs more than the select it replaces.  The share is
    // estimated from the digit range; GKM_RANGE_FUSED=0/1 forces either path.
    bool fused = ks.bits == 2 && span > 0 && (uint64_t)span * kFusedMaxRanks >= (1ull << ob);
    if (const char *e = opt("GKM_RANGE_FUSED")) fused = ks.bits == 2 && span > 0 && e[0] == '1';
    if (fused) {
        uint64_t found = 0;
        rc = d.l0_count(0, L, digit_lo, span, &found, ob);
        if (rc != GK_OK) return rc;
        if (found > 0xFFFFFFFFull) return fail(c, GK_E_ARG, "more k-mers than uint32 start indices can address");
        *n_kept = found;
        if (found == 0) {
            timer_end(c, d.total_slot);
            return GK_OK;
        }
        rc = ensure_elems(c, found + 1, 1);
        if (rc != GK_OK) return rc;
        c->n = found;
        rc = d.init(found);
        if (rc != GK_OK) return rc;
        int in = 0;
        rc = d.l0_start(found, &in);
        return d.run_from(rc, 1, d.width(0), in);
    }
    const uint32_t ntiles = (uint32_t)std::max<uint64_t>((L + kSTile - 1) / kSTile, 1);
    L0Args a{c->sba, 0, L, ks.symbols, d.B, ks.acgt_only};
    a.own_lo = digit_lo;
    a.own_span = span;
    a.own_bits = ob;
    a.pk_code = d.l0a.pk_code;
    a.pk_dol = d.l0a.pk_dol;
    const Dig d0 = dig_at(d.B, 0, d.width(0));
    uint32_t *wave_cnt;
    int slot;
    uint64_t found = 0;
    std::vector<uint64_t> poff, plen;
    if (ks.bits == 2 && !ks.canonical && a.pk_code && ks.symbols <= 32 && a.own_bits <= 32) {
        // the SWAR select over the packed copy: one region per wave (msd0_rsel_kernel)
        const uint64_t ngroups = (L + 31) / 32;
        uint64_t nwv = (uint64_t)d.cus * resident_per_cu(c, (const void *)msd0_rsel_kernel, kRselW * 64) * kRselW;
        const uint64_t gpw = ((ngroups + nwv - 1) / nwv + 63) / 64 * 64;  // whole 64-group steps per wave
        nwv = (ngroups + gpw - 1) / gpw;
        const unsigned nblk = (unsigned)((nwv + kRselW - 1) / kRselW);
        const uint64_t cap = (uint64_t)nblk * kRselW * gpw * 32;  // every wave region is full-size
        if (cap > 0xFFFFFFFFull) return fail(c, GK_E_ARG, "sequence too long for uint32 start indices");
        rc = ensure_elems(c, cap, 1);
        if (rc != GK_OK) return rc;
        GK_TRY_HIP(c, scratch(c, "msd_nd", cap + 64, &d.nd));
        GK_TRY_HIP(c, scratch(c, "sel_wave_cnt", (uint64_t)nblk * kRselW + 1, &wave_cnt));
        const int sh = 32 - a.own_bits;
        const uint32_t lo_w = (uint32_t)((uint64_t)a.own_lo << sh);
        const uint32_t spm1_w = (uint32_t)(((uint64_t)std::min<uint64_t>(a.own_span, 1ull << a.own_bits) << sh) - 1);
        timer_begin(c, "msd_select", &slot);
        timer_units(c, slot, L);
        if (a.own_span == 0) {
            GK_TRY_HIP(c, hipMemsetAsync(wave_cnt, 0, 4 * nwv, c->stream));
        } else {
            hipLaunchKernelGGL(msd0_rsel_kernel, dim3(nblk), dim3(kRselW * 64), 0, c->stream, a, d0, ngroups, gpw, lo_w,
                               spm1_w, wave_cnt, c->keys[1], c->vals[1], d.nd);
        }
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        rc = d.harvest_pieces(wave_cnt, nwv, gpw * 32, slot, &poff, &plen, &found);
    } else {
        // the select over the byte sequence: one region per chunk of tiles (select_launch)
        const uint64_t cap = (uint64_t)ntiles * kSTile;  // every chunk region is full-size
        if (cap > 0xFFFFFFFFull) return fail(c, GK_E_ARG, "sequence too long for uint32 start indices");
        rc = ensure_elems(c, cap, 1);
        if (rc != GK_OK) return rc;
        GK_TRY_HIP(c, scratch(c, "msd_nd", cap + 64, &d.nd));
        GK_TRY_HIP(c, scratch(c, "sel_wave_cnt", (uint64_t)ntiles + 1, &wave_cnt));
        timer_begin(c, "msd_select", &slot);
        timer_units(c, slot, L);
        uint32_t tpw = 1, nchunk = 0;
        if (ks.bits == 2 && ks.canonical) d.select_launch<2, true>(a, d0, ntiles, wave_cnt, &tpw, &nchunk);
        else if (ks.bits == 2) d.select_launch<2, false>(a, d0, ntiles, wave_cnt, &tpw, &nchunk);
        else if (ks.canonical) d.select_launch<4, true>(a, d0, ntiles, wave_cnt, &tpw, &nchunk);
        else d.select_launch<4, false>(a, d0, ntiles, wave_cnt, &tpw, &nchunk);
        GK_TRY_HIP(c, hipGetLastError());
        timer_end(c, slot);
        rc = d.harvest_pieces(wave_cnt, nchunk, (uint64_t)tpw * kSTile, slot, &poff, &plen, &found);
    }
    if (rc != GK_OK) return rc;
    *n_kept = found;
    c->n = found;
    if (found == 0) {
        timer_end(c, d.total_slot);
        return GK_OK;
    }
    uint8_t *nd_keep = d.nd;
    rc = d.init(found);
    if (rc != GK_OK) return rc;
    d.nd = nd_keep;
    d.cur_fmt = MsdDriver::Fmt::KeyStartDigit;  // the select wrote the L0 digit bytes
    // the chunks' regions of keys[1] / vals[1] are the pieces of one bucket, in position order;
    // the first level partitions them into [0, found) of keys[0] / vals[0]
    const std::vector<uint32_t> pb(poff.size(), 0u);
    rc = d.first_level_from_pieces(c->keys[1], c->vals[1], poff.data(), plen.data(), pb.data(), (uint32_t)poff.size(),
                                   0, 0);
    return d.run_from(rc, 1, d.width(0), 0);
}

}  // namespace gkm
