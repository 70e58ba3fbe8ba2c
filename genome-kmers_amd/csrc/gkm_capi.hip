// gkm_capi.hip -- the extern "C" boundary of libgkm.so: lifetime, input, enumerate, gk_sort, the copy,
// locate and view calls, gk_set_option.  (The shard calls: gkm_shard.hip; gk_rank_mode:
// gkm_rankcheck.hip; gk_profile_*: gkm_runtime.hip; the query calls and gk_lcp: their own files.)
//
// Sort strategies:
//   direct   max_kmer_len given and the padded key fits 256 bits: encode once, LSD radix sort.
//   doubling max_kmer_len None (suffix order up to '$', the Kmers default) or a very long bound:
//            prefix doubling over every sba position (gkm_doubling.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>

#include "gkm_internal.h"

namespace gkm {

// ---------------------------------------------------------------------------------------------
// options (gk_set_option): test and tuning overrides of the GKM_* knobs, process-wide
// ---------------------------------------------------------------------------------------------
namespace {
// every knob the library reads through opt(); gk_set_option refuses any other name.  env: the
// operational knobs the environment may also set (transfer, packer, rank fallback, prefetch,
// tracing, mapped buffers); everything else needs gk_set_option.  (GKM_FASTA_CHUNK is not here: the
// FASTA reader, plain C++ beside the library, reads it from the environment itself.)
struct Knob {
    const char *name;
    bool env;
};
constexpr Knob kKnobs[] = {
    // operational
    {"GKM_RANK_BALLOT", true},      {"GKM_PACK_IMPL", true},        {"GKM_PACK_MIN", true},
    {"GKM_PACK_BLOCKS", true},      {"GKM_XFER_THREADS", true},     {"GKM_XFER_HYBRID", true},
    {"GKM_XFER_NUMA", true},        {"GKM_NO_RESIDENT_PACK", true}, {"GKM_PREFETCH_REGIONS", true},
    {"GKM_MSD_TRACE", true},        {"GKM_VMM_CHUNK_MB", true},
    // alternative sort paths that the tests or the benchmark compare
    {"GKM_WIDE_L0", false},         {"GKM_OWN_L0_COMPACT", false},  {"GKM_RANGE_FUSED", false},
    {"GKM_NO_COMPACT", false},      {"GKM_LEVEL_BITS", false},      {"GKM_NO_FUSED_UNIFORM", false},
    {"GKM_NO_MERGE_KEYS", false},   {"GKM_SORT_KEYS_LSD", false},   {"GKM_MSD_KEYS_MIN", false},
    // tests: forced formats and chunk sizes
    {"GKM_TEST_PAIRS", false},      {"GKM_TEST_P88", false},        {"GKM_TEST_CHUNK_TILES", false},
    {"GKM_TEST_SCAN_CHUNK", false}, {"GKM_TEST_SEG_SCAN_MULTI", false}, {"GKM_TEST_CHECK_TILES", false},
    {"GKM_TEST_VMM_MIN_KB", false},
    // gk_lookup (gkm_lookup.hip): forced path (bytes | keys), queries per launch, directory off (0)
    {"GKM_LOOKUP_PATH", false},     {"GKM_LOOKUP_CHUNK", false},    {"GKM_LOOKUP_DIR", false},
    // gk_lookup_mismatch (gkm_mismatch.hip): forced path (bytes | keys), queries per launch
    {"GKM_MISMATCH_PATH", false},   {"GKM_MISMATCH_CHUNK", false},
    // gk_join (gkm_join.hip): forced path (bytes | keys)
    {"GKM_JOIN_PATH", false},
    // gk_screen (gkm_screen.hip): forced path (bytes | keys), bytes of reads per launch
    {"GKM_SCREEN_PATH", false},     {"GKM_SCREEN_CHUNK", false},
    // gk_lcp (gkm_lcp.hip): forced path (bytes | keys)
    {"GKM_LCP_PATH", false},
    // gk_match (gkm_match.hip): forced path (bytes | keys), bytes of reads per launch
    {"GKM_MATCH_PATH", false},      {"GKM_MATCH_CHUNK", false},
    // gk_minimizers (gkm_minimizer.hip): positions a chunk owns
    {"GKM_MINIMIZER_CHUNK", false},
};
const Knob *find_knob(const char *name) {
    for (const Knob &k : kKnobs)
        if (std::strcmp(k.name, name) == 0) return &k;
    return nullptr;
}

std::mutex g_opt_mu;
// the overrides point into g_opt_values, which only grows: a pointer opt() returned stays valid
// whatever gk_set_option does later (the set of values a process ever sets is tiny)
std::set<std::string> g_opt_values;
std::map<std::string, const char *> g_opts;
}  // namespace

const char *opt(const char *name) {
    {
        std::lock_guard<std::mutex> lk(g_opt_mu);
        auto it = g_opts.find(name);
        if (it != g_opts.end()) return it->second;
    }
    const Knob *k = find_knob(name);
    return k && k->env ? std::getenv(name) : nullptr;
}

}  // namespace gkm

using namespace gkm;

// ---------------------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------------------
extern "C" int gk_device_count(int *count) {
    if (!count) return GK_E_ARG;
    hipError_t e = hipGetDeviceCount(count);
    return e == hipSuccess ? GK_OK : GK_E_HIP;
}

extern "C" int gk_create(gk_ctx **out, int device) {
    if (!out) return GK_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GK_E_HIP;
    if (device < 0 || device >= ndev) return GK_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return GK_E_HIP;
    if (int rc = lds_rank_check(device)) return rc;
    gk_ctx *c = new gk_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->counters, 4 * 64) != hipSuccess || hipMalloc(&c->hist, 4 * 256 * kMaxWords * 8) != hipSuccess ||
        hipMalloc(&c->offsets, 4 * 256 * kMaxWords * 8) != hipSuccess || hipMalloc(&c->scalars, 8 * 64) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->hpin), 8 * kHostPinWords, hipHostMallocDefault) != hipSuccess) {
        gk_destroy(c);
        return GK_E_HIP;
    }
    *out = c;
    return GK_OK;
}

extern "C" void gk_destroy(gk_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->pre_stream) hipStreamSynchronize(c->pre_stream);
    xfer_release(c);
    if (c->hpin) hipHostFree(c->hpin);
    if (c->stage_pin) hipHostFree(c->stage_pin);
    for (hipEvent_t e : c->stage_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->pre_ev) hipEventDestroy(e);
    if (c->pre_done) hipEventDestroy(c->pre_done);
    if (c->pre_stream) hipStreamDestroy(c->pre_stream);
    void *bufs[] = {c->sba, c->seg, c->res_code, c->res_dol, c->vals[0], c->vals[1], c->keys[0], c->keys[1], c->status, c->counters,
                    c->hist, c->offsets, c->flags, c->idx_a, c->idx_b, c->ucount, c->cumk, c->tile_sums, c->scalars,
                    c->dhist, c->mask, c->hmask, c->ranks, c->ym, c->yoff, c->oy, c->ot, c->onum,
                    c->mz_pos, c->mz_key, c->mz_strand};
    for (void *b : bufs)
        if (b) dev_free(b);
    for (auto &e : c->scratch)
        if (e.second.first) dev_free(e.second.first);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const char *gk_last_error(gk_ctx *c) { return c ? c->err.c_str() : "null context"; }

extern "C" int gk_sync(gk_ctx *c) {
    if (!c) return GK_E_ARG;
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_stream(gk_ctx *c, void **stream) {
    if (!c || !stream) return GK_E_ARG;
    *stream = (void *)c->stream;
    return GK_OK;
}

// ---------------------------------------------------------------------------------------------
// input
// ---------------------------------------------------------------------------------------------
extern "C" int gk_set_sequence(gk_ctx *c, const uint8_t *sba, uint64_t len, const uint32_t *seg_starts, uint64_t nseg) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!sba || len == 0) return fail(c, GK_E_ARG, "sequence byte array is empty");
    if (!seg_starts || nseg == 0) return fail(c, GK_E_ARG, "sequence_collection is empty");
    if (len > 0xFFFFFFFFull) return fail(c, GK_E_LIMIT, "sequence byte array longer than 2^32-1");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (seg_starts[0] != 0) return fail(c, GK_E_ARG, "first segment must start at 0");
    uint64_t max_len = 0;
    bool internal = false;
    for (uint64_t s = 0; s < nseg; ++s) {
        const uint64_t b = seg_starts[s];
        const uint64_t e = seg_last(seg_starts, nseg, len, s);
        if (s + 1 < nseg && ((uint64_t)seg_starts[s + 1] < b + 2 || (uint64_t)seg_starts[s + 1] > len))
            return fail(c, GK_E_ARG, "segment starts are not strictly increasing by >= 2");
        if (s > 0 && sba[b - 1] != GK_DOLLAR) internal = true;  // separator missing
        if (e < b) return fail(c, GK_E_ARG, "empty segment");
        max_len = std::max<uint64_t>(max_len, e - b + 1);
    }
    const uint64_t padded = ((len + kEncodeTile - 1) / kEncodeTile) * kEncodeTile + kSbaPad;
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->sba), &c->sba_cap, padded));
    GK_TRY_HIP(c, hipMemsetAsync(c->sba + len, GK_DOLLAR, c->sba_cap - len, c->stream));
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->seg), &c->seg_cap, 4 * nseg));
    GK_TRY_HIP(c, hipMemcpyAsync(c->seg, seg_starts, 4 * nseg, hipMemcpyHostToDevice, c->stream));
    c->sba_len = len;
    c->nseg = nseg;
    c->hseg.assign(seg_starts, seg_starts + nseg);
    c->max_seg_len = max_len;
    uint32_t h[2] = {0, 0};  // alphabet classes seen (alphabet_kernel's bits), '$' count
    if (len >= packed_transfer_min()) {
        // 2-bit packed over the link, census on the host, unpacked into the resident sba on the
        // device (gkm_xfer.hip); the stream orders the sort's kernels behind the last unpack, so
        // only the census is waited for
        uint64_t dollars = 0;
        // a sort hint (gk_sort_hint): the L0 pass of gk_sort(k) runs as the sequence lands
        L0Prefetch *pf = nullptr;
        if (c->hint_k && !internal)
            if (int rc = prefetch_plan(c, len, &pf)) return rc;
        if (int rc = packed_transfer(c, sba, len, &h[0], &dollars, pf)) return rc;
        h[1] = (uint32_t)dollars;
    } else {
        GK_TRY_HIP(c, hipMemcpyAsync(c->sba, sba, len, hipMemcpyHostToDevice, c->stream));
        uint32_t *d_flags = reinterpret_cast<uint32_t *>(c->scalars + 8);
        GK_TRY_HIP(c, launch_alphabet(c, d_flags));
        GK_TRY_HIP(c, hipMemcpyAsync(h, d_flags, 8, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    }
    set_kmer_set(c, KmerSet::None);
    if (len < packed_transfer_min()) c->res_pk = false;  // (the packed transfer sets it)
    c->n = 0;
    if (h[0] & 4u) return fail(c, GK_E_ALPHABET, "Sequence contains non-allowed characters!");
    c->acgt = (h[0] & 2u) ? 0 : 1;
    c->internal_dollar = internal || (uint64_t)h[1] != nseg - 1;
    return GK_OK;
}

extern "C" int gk_sort_hint(gk_ctx *c, uint32_t k, uint32_t flags) {
    if (!c) return GK_E_ARG;
    if (flags != 0) return fail(c, GK_E_ARG, "gk_sort_hint: flags must be 0 (forward k-mers)");
    c->hint_k = k;
    return GK_OK;
}

extern "C" int gk_copy_sequence(gk_ctx *c, uint8_t *dst, uint64_t len) {
    if (!c) return GK_E_ARG;
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (len != c->sba_len) return fail(c, GK_E_ARG, "len differs from the loaded sequence length");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    GK_TRY_HIP(c, hipMemcpyAsync(dst, c->sba, len, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_alphabet_is_acgt(gk_ctx *c, int *is_acgt) {
    if (!c || !is_acgt) return GK_E_ARG;
    *is_acgt = c->acgt;
    return GK_OK;
}

extern "C" int gk_resident_packed(gk_ctx *c, int *on) {
    if (!c || !on) return GK_E_ARG;
    *on = c->res_pk ? 1 : 0;
    return GK_OK;
}

extern "C" int gk_set_option(const char *name, const char *value) {
    if (!name || !find_knob(name)) return GK_E_ARG;  // (a retired or misspelt knob fails loudly)
    std::lock_guard<std::mutex> lk(g_opt_mu);
    if (value) g_opts[name] = g_opt_values.insert(value).first->c_str();
    else g_opts.erase(name);
    return GK_OK;
}

// ---------------------------------------------------------------------------------------------
// enumerate (kmers.py:789-861)
// ---------------------------------------------------------------------------------------------
extern "C" int gk_enumerate(gk_ctx *c, uint32_t min_k, uint64_t *n_out) {
    if (!c) return GK_E_ARG;
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (min_k < 1) return fail(c, GK_E_ARG, "min_kmer_len must be greater than zero");
    uint64_t n = 0, shortest = ~0ull;
    for (uint64_t s = 0; s < c->nseg; ++s) {
        const uint64_t l = seg_last(c->hseg.data(), c->nseg, c->sba_len, s) - c->hseg[s] + 1;
        shortest = std::min(shortest, l);
        if (l >= min_k) n += l - min_k + 1;
    }
    if (min_k > shortest) return fail(c, GK_E_ARG, "min_kmer_len must be <= the shortest sequence length");
    if (n > 0xFFFFFFFFull) return fail(c, GK_E_LIMIT, "the size of the required kmers array exceeds the limit set by a uint32");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (min_k != c->pre_k) pre_drop(c);  // (a prefetched L0 serves the enumeration of its k only)
    c->have_starts = false;  // (ensure_elems keeps no starts of the earlier set)
    int rc = ensure_elems(c, n, 1);
    if (rc != GK_OK) return rc;
    c->n = n;
    c->min_k = min_k;
    c->cur = 0;
    // The enumerate output is a pure function of (seg, min_k): it is materialised lazily by the
    // first reader (materialize_starts); the encoder regenerates positions itself.
    set_kmer_set(c, KmerSet::Enumerated);
    if (n_out) *n_out = n;
    return GK_OK;
}

extern "C" int gk_set_start_indices(gk_ctx *c, const uint32_t *src, uint64_t n, uint32_t min_k) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sba) return fail(c, GK_E_STATE, "no sequence loaded");
    if (n > 0 && !src) return fail(c, GK_E_ARG, "null start array");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    c->have_starts = false;  // (ensure_elems keeps no starts of the earlier set)
    int rc = ensure_elems(c, std::max<uint64_t>(n, 1), 1);
    if (rc != GK_OK) return rc;
    c->cur = 0;
    if (n) GK_TRY_HIP(c, hipMemcpyAsync(c->vals[0], src, 4 * n, hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    c->n = n;
    c->min_k = min_k;
    set_kmer_set(c, KmerSet::Given);
    return GK_OK;
}

extern "C" int gk_num_kmers(gk_ctx *c, uint64_t *n) {
    if (!c || !n) return GK_E_ARG;
    *n = c->have_starts ? c->n : 0;
    return GK_OK;
}

// ---------------------------------------------------------------------------------------------
// sort (kmers.py:1624-1731)
// ---------------------------------------------------------------------------------------------
int gkm::ensure_keys(gk_ctx *c) {
    if (!c->keys_valid || !c->keys_stale) return GK_OK;
    // the MSD sort runs on one key word; all words are allocated on first use
    if (int rc = ensure_elems(c, c->n, c->spec.words)) return rc;
    int slot;
    timer_begin(c, "reencode_keys", &slot);
    // multi-word keys of a sorted enumeration: through an enumeration-order table in the free key
    // buffer (one aligned row per k-mer instead of a ~70-byte window at a random position)
    const KeySpec &ks = c->spec;
    // (the table path answers hipErrorNotSupported when it does not apply -- e.g. per-contig k-mer
    // counts that do not add up to n -- and the window gather, always correct, runs instead)
    hipError_t te = hipErrorNotSupported;
    if (c->enum_sorted && ks.words >= 2 && ks.symbols == ks.min_len && ks.symbols <= 64 &&
        (ks.bits == 2 || ks.bits == 4) && c->n >= 4096 && c->key_words_b[c->cur ^ 1] >= ks.words)
        te = launch_encode_table_gather(c, ks, c->vals[c->cur], c->n, c->keys[c->cur], c->keys[c->cur ^ 1],
                                        8 * (uint64_t)c->key_words_b[c->cur ^ 1] * (c->elem_cap + 64));
    if (te == hipErrorNotSupported)
        GK_TRY_HIP(c, launch_encode_gather(c, c->spec, c->vals[c->cur], c->n, c->keys[c->cur]));
    else
        GK_TRY_HIP(c, te);
    timer_end(c, slot);
    c->keys_valid = true;
    c->keys_stale = false;
    return GK_OK;
}

static int sort_direct(gk_ctx *c, const KeySpec &ks) {
    // fixed-length keys (k <= 64) from the enumerated starts: stable MSD in one-word phases (gkm_msd.hip)
    const bool msd = c->enumerated && ks.symbols == ks.min_len && ks.symbols <= 64 && (ks.bits == 2 || ks.bits == 4);
    int rc = ensure_elems(c, c->n, msd ? 1 : ks.words);
    if (rc != GK_OK) return rc;
    if (msd) {
        // a mixed sba (N runs, IUPAC letters): ACGT-only k-mers on 2-bit keys, the rest apart
        bool split = false, keys_final = false;
        if (!c->acgt) {
            rc = split_sort(c, ks, &split, &keys_final);
            if (rc != GK_OK) return rc;
        }
        if (!split)
            rc = prefetch_matches(c, ks, c->n) ? msd_sort_prefetched(c, ks, c->n, false, &keys_final)
                                               : msd_sort(c, ks, c->n, false, &keys_final);
        pre_drop(c);
        if (rc != GK_OK) return rc;
        // the sort that ran says whether it left the sorted keys (a one-word MSD sort: in keys[0]); else ensure_keys
        sort_finished(c, ks, (uint32_t)ks.symbols, ks.canonical != 0, /*keys_stale*/ !keys_final,
                      /*keys_are_ranks*/ false);
        return GK_OK;
    }
    bool hist_ready = false;
    if (c->enumerated && ks.canonical) {  // k > 64: canonical keys of the (ascending) starts
        rc = materialize_starts(c);
        if (rc != GK_OK) return rc;
        int slot;
        timer_begin(c, "encode", &slot);
        GK_TRY_HIP(c, launch_encode_gather(c, ks, c->vals[c->cur], c->n, c->keys[c->cur]));
        timer_end(c, slot);
    } else if (c->enumerated) {
        int slot;
        timer_begin(c, "encode", &slot);
        // (no LSD digit histograms when the MSD path sorts the keys)
        hist_ready = !sort_keys_msd(c, c->n, ks.words, ks.total_bits);
        GK_TRY_HIP(c, launch_encode_positions(c, ks, c->keys[c->cur], c->vals[c->cur], hist_ready ? c->hist : nullptr));
        timer_end(c, slot);
    } else {
        rc = presort_by_start(c);
        if (rc != GK_OK) return rc;
        int slot;
        timer_begin(c, "encode", &slot);
        timer_units(c, slot, c->n);
        GK_TRY_HIP(c, launch_encode_gather(c, ks, c->vals[c->cur], c->n, c->keys[c->cur]));
        timer_end(c, slot);
    }
    rc = sort_keys(c, ks.words, ks.total_bits, hist_ready);
    if (rc != GK_OK) return rc;
    sort_finished(c, ks, (uint32_t)ks.symbols, ks.canonical != 0, /*keys_stale*/ false, /*keys_are_ranks*/ false);
    return GK_OK;
}

namespace gkm {
int quicksort_by_rank(uint64_t *A, uint64_t n);  // gkm_qsort.cpp

// GK_SORT_QUICKSORT_ORDER helpers: the dense group rank of sorted element i is the last group
// whose first sorted index is <= i (binary search over the G group starts), scattered to its start
__global__ __launch_bounds__(256) void qs_rank_scatter_kernel(const uint32_t *__restrict__ S, uint64_t n,
                                                              const uint32_t *__restrict__ gs, uint64_t G,
                                                              uint32_t *__restrict__ rank_of_pos) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = G;  // the last g with gs[g] <= i (gs[0] == 0)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (gs[mid] <= i) lo = mid;
            else hi = mid;
        }
        rank_of_pos[S[i]] = (uint32_t)lo;
    }
}

// one word per original start, in the original order: rank << 32 | start
__global__ __launch_bounds__(256) void qs_pack_kernel(const uint32_t *__restrict__ orig, uint64_t n,
                                                      const uint32_t *__restrict__ rank_of_pos,
                                                      uint64_t *__restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = orig[i];
        out[i] = ((uint64_t)rank_of_pos[s] << 32) | s;
    }
}
}  // namespace gkm

// GK_SORT_QUICKSORT_ORDER, after the device sort: every start's dense group rank from the device's
// group pass, packed on the device with the start in the ORIGINAL start order `orig` (a device
// copy taken before the sort), then numba's quicksort on the host over those words with rank
// comparisons (gkm_qsort.cpp); the result replaces the sorted starts.  Only members of a group
// change places, so keys, head flags and unique counts stay valid.  Host memory: 8 B per k-mer.
static int apply_quicksort_order(gk_ctx *c, std::vector<uint32_t> &orig_host) {
    const uint64_t n = c->n;
    uint64_t G = 0;
    if (int rc = gk_unique_counts(c, &G)) return rc;
    if (int rc = materialize_starts(c)) return rc;
    // the one-off buffers below (4 B per position + 12 B per k-mer) are released on every return
    struct Release {
        gk_ctx *c;
        ~Release() {
            scratch_release(c, "qs_orig");
            scratch_release(c, "qs_rank");
            scratch_release(c, "qs_words");
        }
    } release{c};
    uint32_t *orig, *rank_of_pos;
    uint64_t *words;
    GK_TRY_HIP(c, scratch(c, "qs_orig", n, &orig));
    GK_TRY_HIP(c, hipMemcpyAsync(orig, orig_host.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t>().swap(orig_host);  // (host peak: the 8 B per k-mer below)
    GK_TRY_HIP(c, scratch(c, "qs_rank", c->sba_len + 1, &rank_of_pos));
    GK_TRY_HIP(c, scratch(c, "qs_words", n, &words));
    hipLaunchKernelGGL(qs_rank_scatter_kernel, dim3(grid_of(n)), dim3(256), 0, c->stream, c->vals[c->cur], n, c->idx_b,
                       G, rank_of_pos);
    GK_TRY_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(qs_pack_kernel, dim3(grid_of(n)), dim3(256), 0, c->stream, orig, n, rank_of_pos, words);
    GK_TRY_HIP(c, hipGetLastError());
    std::vector<uint64_t> A(n);
    GK_TRY_HIP(c, hipMemcpyAsync(A.data(), words, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (quicksort_by_rank(A.data(), n) != 0)
        return fail(c, GK_E_UNSUPPORTED, "numba quicksort stack limit (MAX_STACK = 100) exceeded");
    // the starts (low halves) packed in place into the first 4 n bytes of A: element i is read
    // before bytes [4 i, 4 i + 4) are written, and those lie inside elements already read
    unsigned char *S = reinterpret_cast<unsigned char *>(A.data());
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = (uint32_t)A[i];
        std::memcpy(S + 4 * i, &s, 4);
    }
    GK_TRY_HIP(c, hipMemcpyAsync(c->vals[c->cur], S, 4 * n, hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_sort(gk_ctx *c, uint32_t max_kmer_len, uint32_t flags) {
    if (!c) return GK_E_ARG;
    if (flags & ~(GK_SORT_CANONICAL | GK_SORT_QUICKSORT_ORDER)) return fail(c, GK_E_ARG, "unknown gk_sort flags");
    const bool canonical = (flags & GK_SORT_CANONICAL) != 0;
    const bool qorder = (flags & GK_SORT_QUICKSORT_ORDER) != 0;
    if (qorder && canonical)
        return fail(c, GK_E_ARG, "the reference's quicksort tie order exists for forward k-mers only (no canonical sort)");
    if (!c->have_starts) return fail(c, GK_E_STATE, "no k-mers: call gk_enumerate first");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (max_kmer_len != 0 && max_kmer_len < c->min_k) return fail(c, GK_E_ARG, "max_kmer_len is less than min_kmer_len");
    if (canonical && max_kmer_len != c->min_k)
        return fail(c, GK_E_ARG, "canonical k-mers need a fixed length (max_kmer_len == min_kmer_len)");
    if (canonical && (c->acgt ? 2u : 4u) * max_kmer_len > 64u * kMaxWords)
        return fail(c, GK_E_UNSUPPORTED, "canonical k-mers are limited to 256-bit keys");
    if (c->internal_dollar)
        return fail(c, GK_E_NO_BASES, "kmers compared were less than min_kmer_len: the sba holds a '$' inside a segment");
    if (!c->enumerated && c->n > 0) {
        uint32_t *d_bad = reinterpret_cast<uint32_t *>(c->scalars + 12);
        GK_TRY_HIP(c, launch_validate_starts(c, c->vals[c->cur], c->n, c->min_k, d_bad));
        uint32_t bad = 0;
        GK_TRY_HIP(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, GK_E_NO_BASES, "kmers compared were less than min_kmer_len");
    }
    drop_order_views(c);
    const bool from_enum = c->enumerated;
    // only the fixed-length forward sort of the whole enumeration uses a prefetched L0 (sort_direct)
    if (canonical || qorder || max_kmer_len != c->min_k || !from_enum) pre_drop(c);
    int rc;
    // the start order the reference's quicksort starts from: a host copy (4 B per k-mer), so the
    // device sort's memory peak is not raised by it
    std::vector<uint32_t> orig;
    if (qorder && c->n >= 2) {
        if ((rc = materialize_starts(c))) return rc;
        orig.resize(c->n);
        GK_TRY_HIP(c, hipMemcpyAsync(orig.data(), c->vals[c->cur], 4 * c->n, hipMemcpyDeviceToHost, c->stream));
        GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (c->n < 2) {
        rc = materialize_starts(c);
        if (rc != GK_OK) return rc;
        // nothing to order: the sort finished with whatever spec the context had and no keys (the
        // group pass compares bytes)
        sort_finished(c, c->spec, max_kmer_len, canonical, c->keys_stale, c->keys_are_ranks);
        c->keys_valid = false;
        return GK_OK;
    }
    // direct key?
    KeySpec ks{};
    bool direct = false;
    if (max_kmer_len != 0) {
        const int bits = c->acgt ? 2 : 4;
        const bool bounded = max_kmer_len != c->min_k;
        ks = key_spec(bits, max_kmer_len, (bounded && bits == 2) ? bit_width(max_kmer_len) : 0, (int)c->min_k);
        ks.canonical = canonical ? 1 : 0;
        direct = ks.words <= kMaxWords;
    }
    // bounded keys of two or more words (ACGT, min < max, 2 max + bit_width(max) > 64: max >= 30)
    // over a large array that covers most positions: prefix doubling capped at max -- the seed
    // keys, then only the groups still tied -- instead of one LSD pass per 8 bits of the 2-word
    // keys (13 passes, 21 ms for the reference's max-50 workload).  The doubling ranks every
    // position of the sequence, so a subset of user-given starts (n well below the positions)
    // keeps the direct keys.  The sort's keys are then
    // ranks; the key contract stays the direct one: they are re-encoded from the sorted starts
    // when asked for (keys_stale)
    const bool reroute = direct && ks.words >= 2 && !canonical && max_kmer_len != c->min_k && c->acgt &&
                         (from_enum || 2 * c->n >= c->sba_len) && sort_keys_msd(c, c->n, 1, 64);
    if (reroute) direct = false;
    rc = direct ? sort_direct(c, ks) : sort_doubling(c, max_kmer_len);
    if (rc != GK_OK) return rc;
    // (sort_direct and sort_doubling announced their sort: sort_finished)
    // ranks in keys[cur]: the encoded keys are re-derived on demand (ensure_keys)
    if (reroute) sort_finished(c, ks, max_kmer_len, /*canonical*/ false, /*keys_stale*/ true, /*keys_are_ranks*/ false);
    c->enum_sorted = from_enum && direct && ks.symbols == ks.min_len;
    c->starts_materialized = true;
    c->enumerated = false;
    if (qorder && c->n >= 2) {
        if ((rc = apply_quicksort_order(c, orig)) != GK_OK) {
            c->sorted = false;  // the starts are not in the order asked for
            drop_order_views(c);
            return rc;
        }
    }
    return GK_OK;
}

extern "C" int gk_copy_strand_range(gk_ctx *c, uint64_t offset, uint8_t *dst, uint64_t n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->sorted || !c->canonical) return fail(c, GK_E_STATE, "strands need a canonical sort (GK_SORT_CANONICAL)");
    if (offset > c->n || n > c->n - offset) return fail(c, GK_E_ARG, "range outside the k-mer array");
    if (n == 0) return GK_OK;
    if (!dst) return fail(c, GK_E_ARG, "null array");
    GK_TRY_HIP(c, hipSetDevice(c->device));
    if (int rc = materialize_starts(c)) return rc;
    KeySpec ks{};
    ks.bits = c->acgt ? 2 : 4;
    ks.symbols = (int)c->sort_len;
    uint8_t *d;
    GK_TRY_HIP(c, scratch(c, "strands", n, &d));
    GK_TRY_HIP(c, launch_canon_strands(c, ks, c->vals[c->cur] + offset, n, d));
    GK_TRY_HIP(c, hipMemcpyAsync(dst, d, n, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_copy_strands(gk_ctx *c, uint8_t *dst, uint64_t n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);
    if (c->sorted && c->canonical && n != c->n) return fail(c, GK_E_ARG, "n differs from the k-mer count");
    return gk_copy_strand_range(c, 0, dst, n);
}

extern "C" int gk_copy_start_indices(gk_ctx *c, uint32_t *dst, uint64_t n) {
    if (!c) return GK_E_ARG;
    if (!c->have_starts) return fail(c, GK_E_STATE, "no k-mers");
    if (int rc = materialize_starts(c)) return rc;
    if (n != c->n) return fail(c, GK_E_ARG, "n differs from the k-mer count");
    if (n == 0) return GK_OK;
    GK_TRY_HIP(c, hipMemcpyAsync(dst, c->vals[c->cur], 4 * n, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_copy_start_range(gk_ctx *c, uint64_t offset, uint32_t *dst, uint64_t count) {
    if (!c) return GK_E_ARG;
    if (!c->have_starts) return fail(c, GK_E_STATE, "no k-mers");
    if (int rc = materialize_starts(c)) return rc;
    if (offset > c->n || count > c->n - offset) return fail(c, GK_E_ARG, "range outside the k-mer array");
    if (count == 0) return GK_OK;
    GK_TRY_HIP(c, hipMemcpyAsync(dst, c->vals[c->cur] + offset, 4 * count, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

// start index and segment of selected k-mers: starts[kmer_num[i]] and bisect_right(seg, start) - 1
// (sequence_collection.py:76-97), one thread per k-mer, binary search over the resident seg_starts
__global__ __launch_bounds__(256) void locate_kernel(const uint32_t *__restrict__ starts, uint64_t n,
                                                     const uint32_t *__restrict__ seg, uint32_t nseg,
                                                     const uint64_t *__restrict__ nums, uint64_t m,
                                                     uint32_t *__restrict__ sba_idx, uint32_t *__restrict__ seg_of) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = nums[i];
    const uint32_t s = k < n ? starts[k] : 0xFFFFFFFFu;
    uint32_t lo = 0, hi = nseg;  // first segment start > s
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    sba_idx[i] = s;
    seg_of[i] = lo - 1;  // nseg >= 1 and seg[0] == 0, so lo >= 1 for every valid start
}

extern "C" int gk_locate(gk_ctx *c, const uint64_t *kmer_nums, uint64_t m, uint32_t *sba_idx, uint32_t *seg) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->have_starts) return fail(c, GK_E_STATE, "no k-mers");
    if (m == 0) return GK_OK;
    if (!kmer_nums || !sba_idx || !seg) return fail(c, GK_E_ARG, "null array");
    if (int rc = materialize_starts(c)) return rc;
    for (uint64_t i = 0; i < m; ++i)
        if (kmer_nums[i] >= c->n) return fail(c, GK_E_ARG, "kmer_num out of range");
    uint64_t *d_nums;
    uint32_t *d_out;
    GK_TRY_HIP(c, scratch(c, "locate_nums", m, &d_nums));
    GK_TRY_HIP(c, scratch(c, "locate_out", 2 * m, &d_out));
    GK_TRY_HIP(c, hipMemcpyAsync(d_nums, kmer_nums, 8 * m, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(locate_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, c->vals[c->cur], c->n,
                       c->seg, (uint32_t)c->nseg, d_nums, m, d_out, d_out + m);
    GK_TRY_HIP(c, hipGetLastError());
    GK_TRY_HIP(c, hipMemcpyAsync(sba_idx, d_out, 4 * m, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipMemcpyAsync(seg, d_out + m, 4 * m, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    return GK_OK;
}

extern "C" int gk_key_layout(gk_ctx *c, uint32_t *words, uint32_t *bits, uint32_t *symbols) {
    if (!c) return GK_E_ARG;
    if (!c->keys_valid) return fail(c, GK_E_STATE, "no encoded keys: sort first");
    if (words) *words = (uint32_t)c->spec.words;
    if (bits) *bits = c->keys_are_ranks ? 0u : (uint32_t)c->spec.bits;
    if (symbols) *symbols = c->keys_are_ranks ? 0u : (uint32_t)c->spec.symbols;
    return GK_OK;
}

extern "C" int gk_copy_keys(gk_ctx *c, uint64_t *dst, uint64_t n_words) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (!c->keys_valid) return fail(c, GK_E_STATE, "no encoded keys: sort first");
    if (int rc = ensure_keys(c)) return rc;
    const uint64_t W = (uint64_t)c->spec.words;
    if (n_words != W * c->n) return fail(c, GK_E_ARG, "n_words differs from words_per_key * n");
    if (!n_words) return GK_OK;
    // device SoA (word-major) -> host AoS (key-major)
    std::vector<uint64_t> tmp(n_words);
    GK_TRY_HIP(c, hipMemcpyAsync(tmp.data(), c->keys[c->cur], 8 * n_words, hipMemcpyDeviceToHost, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    if (W == 1) {
        std::memcpy(dst, tmp.data(), 8 * n_words);
    } else {
        for (uint64_t i = 0; i < c->n; ++i)
            for (uint64_t w = 0; w < W; ++w) dst[i * W + w] = tmp[w * c->n + i];
    }
    return GK_OK;
}

extern "C" int gk_set_filter_mask(gk_ctx *c, const uint8_t *mask, uint64_t n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->mask), &c->mask_cap, n + 64));
    if (n) GK_TRY_HIP(c, hipMemcpyAsync(c->mask, mask, n, hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    c->mask_n = n;
    return GK_OK;
}

extern "C" int gk_set_group_heads(gk_ctx *c, const uint8_t *heads, uint64_t n) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    GK_TRY_HIP(c, ensure(reinterpret_cast<void **>(&c->hmask), &c->hmask_cap, n + 64));
    if (n) GK_TRY_HIP(c, hipMemcpyAsync(c->hmask, heads, n, hipMemcpyHostToDevice, c->stream));
    GK_TRY_HIP(c, hipStreamSynchronize(c->stream));
    c->hmask_n = n;
    return GK_OK;
}

extern "C" int gk_device_views(gk_ctx *c, void **starts, void **keys, uint64_t *n, uint32_t *words) {
    if (!c) return GK_E_ARG;
    pre_drop(c);  // (the k-mer buffers: a prefetched L0 does not survive)
    if (int rc = materialize_starts(c)) return rc;
    if (keys && c->keys_valid)
        if (int rc = ensure_keys(c)) return rc;
    if (starts) *starts = c->vals[c->cur];
    if (keys) *keys = c->keys[c->cur];
    if (n) *n = c->n;
    if (words) *words = (uint32_t)c->spec.words;
    return GK_OK;
}
