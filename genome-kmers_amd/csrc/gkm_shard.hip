// gkm_shard.hip -- the multi-GPU shard calls of the C ABI (gk_shard_*; genome_kmers/distributed.py):
// the all-to-all exchange's partition and receive-side sort, and the key-range scheme's histogram,
// class-B lists and range sorts.  The sorts themselves are gkm_msd.hip's and gkm_split.hip's.
#include <algorithm>
#include <cstring>

#include "gkm_internal.h"

using namespace gkm;

static int shard_spec(gk_ctx *c, uint32_t k, uint32_t flags, KeySpec *ks) {
    if (flags & ~(GK_SORT_CANONICAL | GK_SHARD_STARTS_ONLY)) return fail(c, GK_E_ARG, "unknown shard flags");
    if ((flags & GK_SHARD_STARTS_ONLY) && ((flags & GK_SORT_CANONICAL) || !c->acgt || k > 32))
        return fail(c, GK_E_UNSUPPORTED, "starts-only shards: forward keys of an A/C/G/T sba with k <= 32");
    if (k == 0 || k > 64) return fail(c, GK_E_ARG, "shard k-mers must have 1 <= k <= 64");
    // (words: the first is exchanged; the rest are re-encoded from the sba)
    *ks = key_spec(c->acgt ? 2 : 4, k, 0, (int)k);
    ks->canonical = (flags & GK_SORT_CANONICAL) ? 1 : 0;
    return GK_OK;
}

extern "C" int gk_shard_bucket_bits(void) { return gkm::msd_radix_bits(); }

extern "C" int gk_shard_partition(gk_ctx *c, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *d_keys,
                                  uint32_t *d_starts, uint64_t cap, uint64_t *h_hist, uint64_t *n_out) {
    const bool starts_only = (flags & GK_SHARD_STARTS_ONLY) != 0;
    if (!c || (!d_keys && !starts_only) || !d_starts || !h_hist || !n_out) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (lo % 32) return fail(c, GK_E_ARG, "shard lo must be a multiple of 32");
    if (hi > c->sba_len) hi = c->sba_len;
    if (c->internal_dollar) return fail(c, GK_E_NO_BASES, "the sba holds a '$' inside a segment");
    KeySpec ks;
    int rc = shard_spec(c, k, flags, &ks);
    if (rc != GK_OK) return rc;
    return msd_shard_partition(c, ks, lo, std::max(hi, lo), starts_only ? nullptr : d_keys, d_starts, cap, h_hist,
                               n_out);
}

// Key-range shards of a mixed sba (N runs, IUPAC letters; k >= 4): the ranges are top-7-bit
// digits of the ACGT-only k-mers' 2-bit keys (split_sort with a SplitRange); other k-mers follow
// the byte-order interval those digits bound.  k < 4: plain 4-bit digits.
static bool range_split(gk_ctx *c, const KeySpec &ks) { return !c->acgt && ks.bits == 4 && ks.symbols >= 4; }

// the 4-bit code of the first ceil(ob / 2) symbols of the smallest ACGT k-mer with top-ob-bit
// digit d (an odd width ends in a half symbol: A or G by the digit's low bit); a range from digit
// 0 has no lower bound, a range to digit 1 << ob no upper one
static uint32_t range_prefix(uint32_t d, bool lower, int ob) {
    const int ns = (ob + 1) / 2;
    if (lower && d == 0) return 0;
    if (d >= (1u << ob)) return 1u << (4 * ns);
    static const uint32_t c4[4] = {1, 3, 5, 12};  // A C G T among '$' A B C D G H K M N R S T V W Y
    const uint32_t dd = (ob & 1) ? d << 1 : d;
    uint32_t v = 0;
    for (int j = 0; j < ns; ++j) v = (v << 4) | c4[(dd >> (2 * (ns - 1 - j))) & 3];
    return v;
}

extern "C" int gk_shard_histogram(gk_ctx *c, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *h_hist,
                                  uint32_t *bits) {
    if (!c || !h_hist || !bits) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (lo % 32) return fail(c, GK_E_ARG, "shard lo must be a multiple of 32");
    if (hi > c->sba_len) hi = c->sba_len;
    if (c->internal_dollar) return fail(c, GK_E_NO_BASES, "the sba holds a '$' inside a segment");
    KeySpec ks;
    int rc = shard_spec(c, k, flags, &ks);
    if (rc != GK_OK) return rc;
    if (range_split(c, ks)) ks = acgt_spec(ks);  // mixed sba: digits of the ACGT-only k-mers
    for (int i = 0; i < 4096; ++i) h_hist[i] = 0;
    int b = 0;
    rc = msd_l0_histogram(c, ks, lo, std::max(hi, lo), h_hist, &b);
    *bits = (uint32_t)b;
    return rc;
}

// the weight of a homopolymer k-mer in the ownership histogram, in 16ths of a sorted k-mer: it
// skips the MSD sort, but is expanded, grouped, keyed and merged (fitted to
// the C4 emulation: 11/16 balances the rank that owns the N runs with the others)
constexpr uint32_t kHomoWeight16 = 11;

extern "C" int gk_shard_class_b(gk_ctx *c, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *h_hist,
                                uint64_t *n_rest, uint64_t *n_runs) {
    if (!c || !h_hist || !n_rest || !n_runs) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, hipSetDevice(c->device));
    *n_rest = *n_runs = 0;
    c->shard_rest.clear();
    c->shard_runs.clear();
    if (c->internal_dollar) return fail(c, GK_E_NO_BASES, "the sba holds a '$' inside a segment");
    KeySpec ks;
    int rc = shard_spec(c, k, flags, &ks);
    if (rc != GK_OK) return rc;
    if (!range_split(c, ks)) return GK_OK;  // no class B: ACGT-only sba, or k < 4
    const int ob = range_own_bits(acgt_spec(ks));
    std::vector<uint32_t> bins(1u << ob);
    for (uint32_t d = 0; d < bins.size(); ++d) bins[d] = range_prefix(d, true, ob);
    rc = split_shard_class_b(c, ks, lo, hi, bins, (ob + 1) / 2, kHomoWeight16, h_hist, &c->shard_rest, &c->shard_runs);
    if (rc != GK_OK) return rc;
    *n_rest = c->shard_rest.size();
    *n_runs = c->shard_runs.size() / 3;
    return GK_OK;
}

extern "C" int gk_shard_class_b_copy(gk_ctx *c, uint32_t *rest, uint64_t n_rest, uint32_t *runs, uint64_t n_runs) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (n_rest != c->shard_rest.size() || 3 * n_runs != c->shard_runs.size())
        return fail(c, GK_E_ARG, "gk_shard_class_b_copy: sizes differ from gk_shard_class_b's");
    if ((n_rest && !rest) || (n_runs && !runs)) return GK_E_ARG;
    if (n_rest) std::memcpy(rest, c->shard_rest.data(), 4 * n_rest);
    if (n_runs) std::memcpy(runs, c->shard_runs.data(), 12 * n_runs);
    return GK_OK;
}

static int shard_sort_range_impl(gk_ctx *c, uint32_t k, uint32_t flags, uint32_t digit_lo, uint32_t digit_hi,
                                 const uint32_t *rest, uint64_t n_rest, const uint32_t *runs, uint64_t n_runs,
                                 bool given, uint64_t *n_kept) {
    if (!c || !n_kept) return GK_E_ARG;
    pre_drop(c);
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (c->internal_dollar) return fail(c, GK_E_NO_BASES, "the sba holds a '$' inside a segment");
    if (digit_lo > digit_hi || digit_hi > 4096u) return fail(c, GK_E_ARG, "digit range outside [0, 4096]");
    KeySpec ks;
    int rc = shard_spec(c, k, flags, &ks);
    if (rc != GK_OK) return rc;
    c->min_k = k;
    set_kmer_set(c, KmerSet::Given);
    bool used = false, keys_final = false;
    if (range_split(c, ks)) {  // mixed sba: ACGT-only k-mers by 2-bit digit, the rest by prefix
        const int ob = range_own_bits(acgt_spec(ks));
        SplitRange rg{digit_lo, digit_hi, range_prefix(digit_lo, true, ob), range_prefix(digit_hi, false, ob), (ob + 1) / 2};
        rg.given = given;
        rg.rest = rest;
        rg.n_rest = n_rest;
        rg.runs = runs;
        rg.n_runs = n_runs;
        rc = split_sort(c, ks, &used, &keys_final, &rg);
        if (rc == GK_OK && !used) rc = fail(c, GK_E_HIP, "key-range split sort not applicable");
        *n_kept = c->n;
    } else {
        rc = msd_sort_range(c, ks, digit_lo, digit_hi, false, n_kept, &keys_final);
    }
    if (rc != GK_OK) return rc;
    // (keys_stale: what the sort just called reported, as in sort_direct, gkm_capi.hip; no k-mers, no keys)
    sort_finished(c, ks, k, ks.canonical != 0, /*keys_stale*/ c->n > 0 && !keys_final, /*keys_are_ranks*/ false);
    return GK_OK;
}

extern "C" int gk_shard_sort_range_b(gk_ctx *c, uint32_t k, uint32_t flags, uint32_t digit_lo, uint32_t digit_hi,
                                     const uint32_t *rest, uint64_t n_rest, const uint32_t *runs, uint64_t n_runs,
                                     uint64_t *n_kept) {
    if ((n_rest && !rest) || (n_runs && !runs)) return GK_E_ARG;
    return shard_sort_range_impl(c, k, flags, digit_lo, digit_hi, rest, n_rest, runs, n_runs, true, n_kept);
}

extern "C" int gk_shard_sort_range(gk_ctx *c, uint32_t k, uint32_t flags, uint32_t digit_lo, uint32_t digit_hi,
                                   uint64_t *n_kept) {
    return shard_sort_range_impl(c, k, flags, digit_lo, digit_hi, nullptr, 0, nullptr, 0, false, n_kept);
}

extern "C" int gk_shard_sort(gk_ctx *c, const uint64_t *d_keys, const uint32_t *d_starts, uint64_t n, uint32_t k,
                             uint32_t flags, const uint64_t *h_piece_off, const uint64_t *h_piece_len,
                             const uint32_t *h_piece_bucket, uint32_t npieces) {
    const bool starts_only = (flags & GK_SHARD_STARTS_ONLY) != 0;
    if (!c || (n && ((!d_keys && !starts_only) || !d_starts || !h_piece_off || !h_piece_len || !h_piece_bucket)))
        return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (n > 0xFFFFFFFFull) return fail(c, GK_E_ARG, "more k-mers than uint32 start indices can address");
    KeySpec ks;
    int rc = shard_spec(c, k, flags, &ks);
    if (rc != GK_OK) return rc;
    for (uint32_t i = 1; i < npieces; ++i)
        if (h_piece_bucket[i] < h_piece_bucket[i - 1]) return fail(c, GK_E_ARG, "pieces must be in bucket order");
    rc = ensure_elems(c, std::max<uint64_t>(n, 1), 1);
    if (rc != GK_OK) return rc;
    c->n = n;
    c->min_k = k;
    set_kmer_set(c, KmerSet::Given);
    bool keys_final = false;
    if (n > 0) {
        rc = msd_shard_sort(c, ks, starts_only ? nullptr : d_keys, d_starts, h_piece_off, h_piece_len, h_piece_bucket,
                            npieces, &keys_final);
        if (rc != GK_OK) return rc;
    } else {
        c->cur = 0;
    }
    // (keys_stale: what the sort just called reported, as in sort_direct, gkm_capi.hip; no k-mers, no keys)
    sort_finished(c, ks, k, ks.canonical != 0, /*keys_stale*/ n > 0 && !keys_final, /*keys_are_ranks*/ false);
    return GK_OK;
}
