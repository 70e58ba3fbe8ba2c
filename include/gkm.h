/*
 * gkm.h -- C ABI of libgkm.so, the MI355X (gfx950) k-mer engine.
 *
 * The reference (mrperkett/genome-kmers v1.0.1) is pure Python + numba and has no FFI; its
 * drop-in boundary is the Kmers / SequenceCollection class surface.  Each entry point below
 * replaces one reference routine (paths relative to the reference's src/genome_kmers/) and is what
 * a ctypes binding inside that class surface binds:
 *
 *   gk_set_sequence        SequenceCollection.forward_sba / _forward_sba_seg_starts as the input
 *                          contract (sequence_collection.py:531-576, 663-726, 155-187); H2D copy.
 *   gk_enumerate           Kmers._initialize_single_pass / _get_unfiltered_kmer_count (kmers.py:789-861)
 *   gk_sort                Kmers.sort + get_is_less_than_func (kmers.py:1624-1731), numba quicksort
 *   gk_copy_start_indices  Kmers.kmer_sba_start_indices read-back (kmers.py:811, 1648)
 *   gk_set_start_indices   assigning Kmers.kmer_sba_start_indices (kmers.py:724, 1462, 1522)
 *   gk_group_hist          get_kmer_group_size_hist (kmers.py:454-520) behind Kmers.get_kmer_count
 *                          (kmers.py:994-1083) and Kmers.get_kmer_group_counts (kmers.py:1085-1178)
 *   gk_group_members       kmer_info_by_group_generator (kmers.py:523-648) behind Kmers.get_kmers
 *                          (kmers.py:869-992)
 *   gk_unique_counts       the (unique k-mer, multiplicity) view of the sorted groups (kmers.py:597-625)
 *   gk_copy_keys           encoded k-mers (no reference counterpart: the reference compares bytes)
 *   gk_locate              the start / record lookups behind get_kmer_info (kmers.py:1180-1264)
 *   gk_shard_partition,    one GPU's share of Kmers.sort under torch.distributed (no reference
 *   gk_shard_sort          counterpart: the reference is single-process, kmers.py:1644-1648)
 *   gk_fasta_open,         SequenceCollection._get_fasta_stats + _load_forward_sba_from_fasta
 *   gk_fasta_fill          (sequence_collection.py:476-576): FASTA -> sba on the host, multithreaded
 *
 * Conventions: every function returns GK_OK (0) or a negative gk_status; gk_last_error(ctx)
 * describes the last failure.  Host pointers are borrowed for the duration of the call only.
 * Device memory is owned by the context and freed by gk_destroy.  A context is bound to one HIP
 * device and one stream; it is not thread-safe.  Work is stream-ordered: functions that return
 * data to the host synchronise the stream, others may return before the device finishes
 * (gk_sync waits).
 */
#ifndef GKM_H
#define GKM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gk_ctx gk_ctx;
typedef struct gk_fasta gk_fasta;

enum gk_status {
    GK_OK = 0,
    GK_E_ARG = -1,          /* invalid argument                                             */
    GK_E_HIP = -2,          /* HIP runtime error                                             */
    GK_E_OOM = -3,          /* device allocation failed                                      */
    GK_E_UNSUPPORTED = -4,  /* configuration not supported by the device path                */
    GK_E_ALPHABET = -5,     /* byte outside {A,B,C,D,G,H,K,M,N,R,S,T,V,W,Y,$}                */
    GK_E_STATE = -6,        /* call out of order (e.g. sort before set_sequence)             */
    GK_E_FILTER = -7,       /* a built-in filter raised (see gk_filter_error)                */
    GK_E_LIMIT = -8,        /* more than 2^32-1 k-mers (kmers.py:805-808)                     */
    GK_E_NO_BASES = -9,     /* comparator found no valid base (kmers.py:368-369)             */
    GK_E_IO = -10,          /* a file could not be opened / mapped                           */
    GK_E_FASTA_NAME = -11,  /* a header line with no name token (IndexError in the reference) */
    GK_E_FASTA_LAYOUT = -12,/* the sba would not be exactly full (sequence_collection.py:565)   */
};

/* built-in k-mer filters (kmers.py:14-259); evaluated on the device */
enum gk_filter_kind {
    GK_FILTER_KEEP_ALL = 0,      /* kmer_filter_keep_all                       kmers.py:14-16   */
    GK_FILTER_LENGTH = 1,        /* gen_kmer_length_filter_func(p0=min_len)    kmers.py:19-34   */
    GK_FILTER_HOMOPOLYMER = 2,   /* gen_kmer_homopolymer_filter_func(p0=max_h, p1=kmer_len)  :37-100 */
    GK_FILTER_GC = 3,            /* gen_kmer_gc_content_filter_func(p0=min_count, p1=max_count, p2=kmer_len) :103-192 */
    GK_FILTER_NO_AMBIGUOUS = 4,  /* gen_no_ambiguous_bases_filter(p0=kmer_len) kmers.py:195-229 */
    GK_FILTER_CRISPR_NGG = 5,    /* crispr_ngg_pam_filter                      kmers.py:232-259 */
    GK_FILTER_MASK = 6,          /* per-sorted-position byte mask from gk_set_filter_mask      */
};

/* filter error codes reported through gk_filter_error (match the reference's raise sites) */
enum gk_filter_error {
    GK_FERR_NONE = 0,
    GK_FERR_HOMO_LEN = 1,    /* kmers.py:66-69 / 83-86  "The kmer_len (..) requested is too large for kmer_sba_start_idx (..)" */
    GK_FERR_GC_LEN = 2,      /* kmers.py:176-179        "... too larger for kmer_sba_start_idx (..)"                        */
    GK_FERR_GC_OOB = 3,      /* read past the end of the sba (undefined behaviour in numba)                                */
    GK_FERR_AMBIG_LEN = 4,   /* kmers.py:212-213        "kmer_len (..) is invalid. It extends beyond len(sba)"              */
    GK_FERR_AMBIG_SEG = 5,   /* kmers.py:220-221        "end of segment was reached. kmer_len (..) invalid."                */
    GK_FERR_CRISPR_LEN = 6,  /* kmers.py:252-253        "The guide defined at this start index extends beyond the sba"      */
};

typedef struct gk_filter {
    int32_t kind;          /* gk_filter_kind */
    int32_t pad;
    int64_t p0, p1, p2;
} gk_filter;

/* gk_sort flags */
#define GK_SORT_DEFAULT 0u
/* Canonical k-mers (C5; this build's extension -- the reference defines none, kmers.py:689-696):
 * sort by min(k-mer, reverse complement) under the reference's byte order, with the reference's
 * IUPAC complement (sequence_collection.py:402-433).  Fixed length only (min_kmer_len ==
 * max_kmer_len); groups, counts and keys then refer to the canonical k-mers. */
#define GK_SORT_CANONICAL 1u
/* The reference's default tie order (Kmers.sort: numba quicksort, break_ties=False,
 * kmers.py:1624-1652): the device sorts, then numba's quicksort runs on the host over the original
 * start order comparing the device's group ranks (gkm_qsort.cpp) -- bit-exact with the reference,
 * equal k-mers included.  Host-bound (8 B of host memory per k-mer: the device hands the host
 * rank << 32 | start per start); not with GK_SORT_CANONICAL. */
#define GK_SORT_QUICKSORT_ORDER 2u

/* ---- lifetime ------------------------------------------------------------------------------ */
int gk_create(gk_ctx **out, int device);
void gk_destroy(gk_ctx *ctx);
const char *gk_last_error(gk_ctx *ctx);
int gk_sync(gk_ctx *ctx);
int gk_device_count(int *count);
/* Partition ranking of the sort on ctx's device.  Every stable partition ranks an item by one
 * returning LDS atomic, which relies on gfx950 applying same-address lanes in lane order;
 * gk_create checks that on every device it opens and, where it does not hold (or GKM_RANK_BALLOT=1
 * is set), switches to a ballot-match ranking: the same order, slower.  mode: -1 = query only,
 * 0 = the device's checked default, 1 = ballot-match forced (tests).  *active (may be NULL):
 * 1 if ballot-match ranking is in use afterwards, else 0. */
int gk_rank_mode(gk_ctx *ctx, int mode, int *active);

/* ---- input contract ------------------------------------------------------------------------- */
/* sba: ASCII bases, contigs joined by '$' (36), no trailing '$'; seg_starts: ascending uint32. */
int gk_set_sequence(gk_ctx *ctx, const uint8_t *sba, uint64_t len, const uint32_t *seg_starts, uint64_t nseg);
/* The transfer: inputs of >= 16 MiB (GKM_PACK_MIN) cross the link 2-bit packed wherever a 64 KiB
 * block is pure A/C/G/T and raw elsewhere, packed by up to 16 host threads (AVX2) and unpacked
 * into the resident ASCII sba on the device (gkm_xfer.hip); the alphabet check runs on the host
 * during the packing.  gk_copy_sequence reads the resident sba back (len = the loaded length). */
int gk_copy_sequence(gk_ctx *ctx, uint8_t *dst, uint64_t len);
/* Sort hint (no reference counterpart: the reference has no transfer; Kmers(sc, k, k) followed by
 * Kmers.sort(), kmers.py:656-760, 1624-1652, is the call pattern it serves).  While k != 0, every
 * later gk_set_sequence that crosses the link packed (>= GKM_PACK_MIN bytes, any number of contigs)
 * also runs the first pass of gk_sort(k) -- the L0 partition of the A/C/G/T-only k-mers by their top
 * key bits -- over regions of the sequence as they land, on a stream of its own; the next
 * gk_enumerate(k) + gk_sort(k, 0) of the whole enumeration then starts from its buckets (same
 * result, less time after the transfer): on an A/C/G/T sba they are the sort's own L0, on a mixed
 * one (N runs, IUPAC letters) the L0 of the split sort's A/C/G/T-only class.
 * Any other call that uses the k-mer buffers drops the prefetched pass.  k = 0 clears the hint;
 * flags must be 0.  Hints outside 8 <= k <= 32 are ignored. */
int gk_sort_hint(gk_ctx *ctx, uint32_t k, uint32_t flags);
/* 1 if the loaded sba holds only {A,C,G,T,$} (2-bit keys), 0 otherwise (4-bit keys) */
int gk_alphabet_is_acgt(gk_ctx *ctx, int *is_acgt);
/* 1 if the last gk_set_sequence left the 2-bit packed copy of the sequence resident beside the sba
 * (the packed transfer: the L0 passes of the sort read it, 0.375 B per position), else 0.  No
 * reference counterpart (the reference has no transfer). */
int gk_resident_packed(gk_ctx *ctx, int *on);
/* Test and tuning overrides of the library's GKM_* knobs, process-wide (no reference counterpart):
 * value NULL clears the override.  The library keeps one table of the knobs it reads (kKnobs,
 * gkm_capi.hip); a name that is not in it -- unknown, misspelt or retired -- is refused with
 * GK_E_ARG.  Only the operational knobs (GKM_RANK_BALLOT, GKM_PACK_IMPL, GKM_PACK_MIN,
 * GKM_PACK_BLOCKS, GKM_XFER_THREADS, GKM_XFER_HYBRID, GKM_XFER_NUMA, GKM_NO_RESIDENT_PACK,
 * GKM_PREFETCH_REGIONS, GKM_MSD_TRACE, GKM_VMM_CHUNK_MB) are also read from the environment; every
 * other knob -- alternative sort paths, forced formats, test-only chunk sizes -- is reachable only
 * through this call.  (GKM_FASTA_CHUNK of the FASTA parser is an environment variable only.) */
int gk_set_option(const char *name, const char *value);

/* ---- enumerate / sort ------------------------------------------------------------------------ */
/* every start with >= min_kmer_len bases before '$' / end, contig by contig, ascending */
int gk_enumerate(gk_ctx *ctx, uint32_t min_kmer_len, uint64_t *n_out);
/* replace the start indices with host-provided ones (any order, each must be a valid start) */
int gk_set_start_indices(gk_ctx *ctx, const uint32_t *src, uint64_t n, uint32_t min_kmer_len);
/*
 * Sort the start indices by the k-mer at each start, compared as compare_sba_kmers_lexicographically
 * with max_kmer_len (0 = None: compare up to the '$' that ends the contig).  Equal k-mers are
 * ordered by start index (the reference's break_ties=True order, kmers.py:1710-1711).
 */
int gk_sort(gk_ctx *ctx, uint32_t max_kmer_len, uint32_t flags);
int gk_num_kmers(gk_ctx *ctx, uint64_t *n);
int gk_copy_start_indices(gk_ctx *ctx, uint32_t *dst, uint64_t n);
/* start indices [offset, offset + count) of the current order (Kmers.get_kmer_str, kmers.py:1604) */
int gk_copy_start_range(gk_ctx *ctx, uint64_t offset, uint32_t *dst, uint64_t count);
/* encoded keys of the sorted k-mers: words_per_key uint64 words per k-mer, most significant first */
int gk_key_layout(gk_ctx *ctx, uint32_t *words_per_key, uint32_t *bits_per_symbol, uint32_t *symbols);
int gk_copy_keys(gk_ctx *ctx, uint64_t *dst, uint64_t n_words);
/* after a GK_SORT_CANONICAL sort: dst[i] = 1 if the reverse complement of sorted k-mer i is its
 * canonical form (strictly smaller than the k-mer), else 0 (the k-mer itself, or a palindrome) */
int gk_copy_strands(gk_ctx *ctx, uint8_t *dst, uint64_t n);
/* the same for the sorted positions [offset, offset + count) only (the hits of a gk_lookup range) */
int gk_copy_strand_range(gk_ctx *ctx, uint64_t offset, uint8_t *dst, uint64_t count);

/* ---- groups ---------------------------------------------------------------------------------- */
/* mask for GK_FILTER_MASK: one byte per position of the current start-index order */
int gk_set_filter_mask(gk_ctx *ctx, const uint8_t *mask, uint64_t n);
/* Group boundaries decided by a caller's comparison (a custom kmer_comparison_func the device cannot
 * run, kmers.py:285-303, 597-601): heads[i] = 1 if the k-mer at position i of the current order
 * differs from the previous VALID k-mer (passing the filter), 0 if it is equal; read at valid
 * positions only, the first valid k-mer always starts a group.  Used by gk_group_hist /
 * gk_group_members called with is_sorted = GK_GROUPS_FROM_HEADS. */
int gk_set_group_heads(gk_ctx *ctx, const uint8_t *heads, uint64_t n);
#define GK_GROUPS_FROM_HEADS 2
/*
 * Histogram of group sizes over k-mers passing `filter`; groups are runs of equal k-mers under
 * compare_sba_kmers_lexicographically(kmer_len) (kmer_len < 0 = None) when is_sorted, else every
 * k-mer is its own group (compare_sba_kmers_always_less_than); is_sorted = GK_GROUPS_FROM_HEADS: the
 * groups gk_set_group_heads described.  max_group_size < 0 = None.
 * hist has max_counts_bin + 1 entries.  On GK_E_FILTER, *err_code / *err_idx name the failing
 * filter check and the SBA index of the first (in start-index order) k-mer that raised.
 */
int gk_group_hist(gk_ctx *ctx, int is_sorted, int64_t kmer_len, const gk_filter *filter, int64_t min_group_size,
                  int64_t max_group_size, int64_t max_counts_bin, int64_t *hist, int64_t *total,
                  int32_t *err_code, uint64_t *err_idx);
/*
 * The first yield_first_n (< 0 = None) members of every qualifying group, in generator order:
 * (kmer_num, group_size_yielded, group_size_total).  Two calls: with kmer_num == NULL only
 * *n_out is set; then call again with arrays of at least *n_out entries.
 */
int gk_group_members(gk_ctx *ctx, int is_sorted, int64_t kmer_len, const gk_filter *filter, int64_t min_group_size,
                     int64_t max_group_size, int64_t yield_first_n, uint64_t *kmer_num, uint32_t *size_yielded,
                     uint32_t *size_total, uint64_t capacity, uint64_t *n_out, int32_t *err_code, uint64_t *err_idx);
/* distinct k-mers of the sorted order (kmer_len = sort length): first sorted index and multiplicity
 * of each, computed and kept in HBM (after a one-word sort, one selection pass over the sort's
 * group heads writes both); gk_copy_unique copies them out, gk_device_unique exposes them.
 * Together with the sorted starts and keys (gk_device_views) this is the unique/count product. */
int gk_unique_counts(gk_ctx *ctx, uint64_t *n_unique);
int gk_copy_unique(gk_ctx *ctx, uint64_t *group_start, uint32_t *count, uint64_t n);
/* device pointers of the unique output: group_start uint32[n_unique], count uint32[n_unique] */
int gk_device_unique(gk_ctx *ctx, void **group_start, void **count, uint64_t *n_unique);

/* ---- device views / timing (bench + multi-GPU orchestration) --------------------------------- */
/* device pointers of the current sorted start indices and keys (valid until the next call); with
 * keys != NULL the keys are materialised first if the sort left them stale (multi-word keys, mixed
 * alphabets: a re-encode from the sorted starts); a one-word sort writes them in sorted order */
int gk_device_views(gk_ctx *ctx, void **starts, void **keys, uint64_t *n, uint32_t *words_per_key);
/* enable per-kernel HIP-event timing; gk_profile_report writes a JSON object to buf */
int gk_profile_enable(gk_ctx *ctx, int on);
int gk_profile_report(gk_ctx *ctx, char *buf, uint64_t buflen);
/* stream handle of the context (hipStream_t), for interop */
int gk_stream(gk_ctx *ctx, void **stream);

/* ---- multi-GPU shards (one process per GPU; the exchange is the caller's all-to-all) --------- */
/* number of top key bits the shard buckets are cut on (buckets = 1 << bits) */
int gk_shard_bucket_bits(void);
/*
 * Send side: encode the fixed-length k-mers (length k <= 64, no '$') that start in sequence
 * positions [lo, hi) (lo a multiple of 32) and partition them stably by their top
 * gk_shard_bucket_bits() key bits into the caller's DEVICE buffers d_keys / d_starts (capacity
 * cap >= count + 1), in ascending bucket order.  d_keys holds each k-mer's FIRST key word (the
 * first 64 / bits symbols); later words are re-encoded from the sba by the receiver.  flags:
 * 0 or GK_SORT_CANONICAL (the same on every rank and in gk_shard_sort).  h_hist[1 << bits] receives the bucket sizes, *n_out the count.
 * Returns after the device work is complete (the buffers can go straight to another stream).
 */
int gk_shard_partition(gk_ctx *ctx, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *d_keys,
                       uint32_t *d_starts, uint64_t cap, uint64_t *h_hist, uint64_t *n_out);
/* Shard flag (round 6): only the start indices cross the exchange -- 4 B per k-mer instead of 12.
 * gk_shard_partition writes d_starts only (d_keys may be NULL); gk_shard_sort ignores d_keys and
 * re-derives every received k-mer's key from its own resident copy of the sequence (every rank holds
 * the whole sba, as the key-range shards do).  Forward keys of an A/C/G/T sba with k <= 32 only
 * (GK_E_UNSUPPORTED otherwise); the same flag on every rank. */
#define GK_SHARD_STARTS_ONLY 4u
/*
 * Receive side: sort n received (key, start) pairs in DEVICE buffers, given as npieces pieces
 * (offset, length, bucket) listed in ascending bucket order; the pieces of one bucket are listed
 * in ascending start order (source rank order).  The context then holds the sorted k-mers as if
 * gk_sort(k) had run on them: starts, keys, unique counts and group passes work as usual.
 * The buffers must be complete when the call is made (work queued on another stream must have
 * been synchronised by the caller).
 */
int gk_shard_sort(gk_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_starts, uint64_t n, uint32_t k,
                  uint32_t flags, const uint64_t *h_piece_off, const uint64_t *h_piece_len, const uint32_t *h_piece_bucket,
                  uint32_t npieces);

/*
 * Key-range shards: multi-GPU with NO data exchange.  Every rank holds the whole sba (as in the
 * all-to-all scheme above); rank r keeps the k-mers whose top key digit lies in its digit range and
 * sorts them, so the ranks' outputs concatenated in rank order are the single-GPU gk_sort order
 * (kmers.py:1624-1652 with break_ties=True, kmers.py:1710-1711).  Replaces the same reference call
 * as gk_sort; the reference has no multi-process path.
 * gk_shard_histogram: histogram of the ownership digits -- the top *bits key bits, 12 for 2-bit
 * keys (k >= 6), 8 for 4-bit keys -- (h_hist[4096], entries >= 1 << *bits are 0) of the
 * fixed-length k-mers starting in [lo, hi) (lo a multiple of 32); on a mixed sba the digits of
 * the ACGT-only k-mers.  Each rank counts its position share, the caller sums the histograms over
 * ranks (an all-reduce of 1 << *bits counts, 32 KiB as int64) and cuts the digits into contiguous
 * ranges of about n / N k-mers: 4096 digits let a hot digit of a skewed genome be split finely.
 * gk_shard_sort_range: sort every k-mer of the sba whose ownership digit d has digit_lo <= d < digit_hi;
 * *n_kept receives their number and the context then holds them as after gk_sort(k).
 */
int gk_shard_histogram(gk_ctx *ctx, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *h_hist,
                       uint32_t *bits);
int gk_shard_sort_range(gk_ctx *ctx, uint32_t k, uint32_t flags, uint32_t digit_lo, uint32_t digit_hi,
                        uint64_t *n_kept);
/* Key-range shards of a mixed sba (N runs, IUPAC letters) without a whole-sequence class-B scan
 * per rank:
 * gk_shard_class_b: the class-B k-mers (some non-ACGT letter) STARTING in [lo, hi) -- the rank's
 *   position share -- kept in the context as host lists in start order: n_rest non-homopolymer
 *   starts and n_runs homopolymer runs (first start, count, canonical letter: three uint32 each);
 *   their ownership digits are ADDED to h_hist (gk_shard_histogram's bins; a homopolymer k-mer
 *   weighs 11/16), so the all-reduced histogram balances them too.  An ACGT-only sba gives 0, 0.
 * gk_shard_class_b_copy: the two lists out (sizes as returned).
 * gk_shard_sort_range_b: gk_shard_sort_range with the class-B k-mers of the WHOLE sba given as the
 *   concatenation, in rank order, of every rank's lists (all-gathered): the rank keeps those in its
 *   interval instead of scanning the sequence for them. */
int gk_shard_class_b(gk_ctx *ctx, uint64_t lo, uint64_t hi, uint32_t k, uint32_t flags, uint64_t *h_hist,
                     uint64_t *n_rest, uint64_t *n_runs);
int gk_shard_class_b_copy(gk_ctx *ctx, uint32_t *rest, uint64_t n_rest, uint32_t *runs, uint64_t n_runs);
int gk_shard_sort_range_b(gk_ctx *ctx, uint32_t k, uint32_t flags, uint32_t digit_lo, uint32_t digit_hi,
                          const uint32_t *rest, uint64_t n_rest, const uint32_t *runs, uint64_t n_runs,
                          uint64_t *n_kept);

/* Location of selected k-mers for Kmers.get_kmers(kmer_info_to_yield="full") (kmers.py:1180-1264):
 * sba_idx[i] = kmer_sba_start_indices[kmer_nums[i]] and seg[i] = the segment holding it
 * (bisect_right over the segment starts, sequence_collection.py:76-97), computed on the device
 * against the resident starts -- the host never needs the whole start array. */
int gk_locate(gk_ctx *ctx, const uint64_t *kmer_nums, uint64_t m, uint32_t *sba_idx, uint32_t *seg);

/* Batch k-mer lookup in the sorted order (no reference routine: the reference offers no search; the
 * comparison is its compare_sba_kmers_lexicographically, kmers.py:306-397).  queries: m x qlen ASCII
 * bytes, row-major, host memory, letters of the sba alphabet without '$'.  Sorted position i matches
 * query j when compare(sba, query_j, starts[i], 0, max_kmer_len=qlen) == 0: all qlen bytes at
 * starts[i] equal the query's and none is '$' or past the end (a k-mer that meets its contig's end
 * first compares less).  first[j] = the number of sorted k-mers that compare less than query j (its
 * insertion point when it is absent), count[j] = the number that match: the matches are the sorted
 * positions [first[j], first[j] + count[j]).  1 <= qlen <= the sort length K (a prefix range for
 * qlen < K; any qlen after a sort with max_kmer_len None).  After GK_SORT_CANONICAL only qlen == K,
 * and the query stands for min(query, reverse complement): a query and its reverse complement give the
 * same range.  After a shard sort the answers refer to the rank's own k-mers.  Synchronises the stream.
 * GK_E_STATE: no sequence, or not sorted; GK_E_ARG: qlen == 0, qlen > K, canonical with qlen != K,
 * null arrays; GK_E_ALPHABET: a query byte outside the alphabet (checked before any launch; the
 * message names the query and the byte).  m == 0 returns GK_OK and touches nothing. */
int gk_lookup(gk_ctx *ctx, const uint8_t *queries, uint64_t m, uint32_t qlen, uint64_t *first, uint32_t *count);

/* K-mer search with mismatches (no reference routine: the reference offers no search; "end of contig"
 * is its comparator's, kmers.py:306-397).  A scan, not a search: every position of the CURRENT
 * start-index order -- sorted, unsorted, canonical, a shard's, or one given with gk_set_start_indices;
 * no sort is needed -- is compared with every query.  queries: m x qlen ASCII bytes, row-major, host
 * memory, letters of the sba alphabet without '$' (gk_lookup's rule and GK_E_ALPHABET message).
 * Position i takes part when the qlen bytes at starts[i] hold no '$' and do not run past the end (a
 * k-mer that meets its contig's end first matches at no distance, as it never matches in gk_lookup);
 * its distance to query j is the number of byte positions that differ, by plain byte inequality ('N'
 * against 'A' is a mismatch, 'N' against 'N' a match: no IUPAC compatibility).  With
 * GK_MISMATCH_BOTH_STRANDS each position is also compared with the reverse complement of the query
 * (the reference's IUPAC complement, sequence_collection.py:402-433) -- the reverse complement of the
 * k-mer against the query -- reported as strand 1, the query as given as strand 0; a position that
 * qualifies on both strands is reported on both.
 * counts[j * (max_mismatches + 1) + d] = the number of (position, strand) pairs at distance exactly d
 * from query j, d in [0, max_mismatches]; *n_hits = their sum, always written.  Hits in two calls, as
 * gk_group_members: with hit_query == NULL only counts and *n_hits; otherwise all four hit arrays
 * are non-null and capacity >= *n_hits (the device's record buffer is sized from the hits found, not
 * from capacity: a search with more than 2^20 hits scans twice), and hit t is query hit_query[t] against position hit_kmer_num[t] of the
 * current order (gk_locate's numbering) at distance hit_mismatches[t] on strand hit_strand[t], in
 * ascending (query, kmer_num, strand) whatever the device's scheduling.  1 <= qlen <= 32,
 * max_mismatches <= qlen, m <= 2^32 (hit_query is 32 bits wide); qlen is not tied to the sort length.
 * Synchronises the stream.
 * GK_E_ARG: a null context, null queries / counts / n_hits / hit arrays, qlen or max_mismatches out of
 * range, m > 2^32, unknown flag bits, capacity < *n_hits (the message names the number); GK_E_STATE: no
 * sequence or no start indices; GK_E_ALPHABET: a query byte outside the alphabet.  m == 0 returns
 * GK_OK with *n_hits = 0 and touches nothing else. */
#define GK_MISMATCH_BOTH_STRANDS 1u
int gk_lookup_mismatch(gk_ctx *ctx, const uint8_t *queries, uint64_t m, uint32_t qlen, uint32_t max_mismatches,
                       uint32_t flags, uint64_t *counts, uint32_t *hit_query, uint64_t *hit_kmer_num,
                       uint8_t *hit_mismatches, uint8_t *hit_strand, uint64_t capacity, uint64_t *n_hits);

/* Join of two sorted contexts (no reference routine: the reference holds one genome at a time; equality
 * and order are its compare_sba_kmers_lexicographically at the common sort length K, kmers.py:306-397,
 * of the canonical forms -- gkm_canon.h -- after GK_SORT_CANONICAL on both sides).  Every distinct
 * k-mer of a -- entry u of a's unique view, gk_unique_counts, which gk_join computes on either side
 * when it is not valid -- is looked up in b: b_count[u] = its multiplicity in b, b_first[u] = the number
 * of b's sorted k-mers that compare less than it (its insertion point when b_count[u] == 0; gk_lookup's
 * convention).  The result is aligned with gk_copy_unique(a), stays in context a as device uint32
 * arrays (a snapshot of b) and is dropped wherever a's unique view is dropped (a sort, new starts, a new
 * sequence, a group pass).  stats (may be NULL): integer sums, the same on every run and on both paths.
 * a == b is allowed (b_count == count, b_first == group_start); an empty side gives GK_OK and zeros.
 * b's stream is synchronised before a's stream reads b's buffers; the work runs on a's stream, which
 * the call synchronises.  Two paths with the same answers: a streaming merge of the two unique views'
 * keys when both contexts hold final one-word 2-bit forward keys (A/C/G/T only, K <= 32, forward
 * order), else one search per distinct k-mer of a over b's sorted starts comparing sequence bytes
 * (mixed alphabets on either side, K > 32, canonical orders); GKM_JOIN_PATH = bytes | keys
 * (gk_set_option) forces one, keys where it does not apply: GK_E_UNSUPPORTED.
 * GK_E_ARG: a null context, contexts on different devices, flags != 0, different sort lengths, one side
 * canonical and the other not; GK_E_STATE: a side without a sequence or not sorted;
 * GK_E_UNSUPPORTED: sort length 0 (None), or a side whose min_kmer_len differs from its sort length
 * (k-mers cut short by a contig end).  Each message names the values. */
typedef struct gk_join_stats {
    uint64_t n_distinct_a, n_distinct_b;   /* distinct k-mers of each side                          */
    uint64_t n_shared;                      /* distinct k-mers present in both                       */
    uint64_t occ_a_shared, occ_b_shared;    /* occurrences in A, in B, of the shared k-mers          */
    uint64_t occ_min;                       /* sum over shared k-mers of min(count in A, count in B) */
} gk_join_stats;
int gk_join(gk_ctx *a, gk_ctx *b, uint32_t flags, gk_join_stats *stats);
/* the result of the last gk_join(ctx, ...): copied out (b_first widened as gk_copy_unique's group starts;
 * n must equal ctx's distinct count, GK_E_ARG otherwise; either array may be NULL), or as device
 * pointers uint32[*n].  GK_E_STATE without a valid join. */
int gk_copy_join(gk_ctx *a, uint64_t *b_first, uint32_t *b_count, uint64_t n);
int gk_device_join(gk_ctx *a, void **b_first, void **b_count, uint64_t *n);
/* Writes the filter mask of GK_FILTER_MASK on the device (as gk_set_filter_mask would, one byte per
 * sorted position): 1 where the k-mer at the position is absent from b (GK_JOIN_KEEP_ABSENT) or
 * present in b (GK_JOIN_KEEP_PRESENT) by the last gk_join, else 0; the cost per position does not
 * depend on the group's size.  Any other keep: GK_E_ARG; GK_E_STATE without a valid join.  The group
 * pass that then reads the mask drops the join with the unique view. */
#define GK_JOIN_KEEP_ABSENT 1
#define GK_JOIN_KEEP_PRESENT 2
int gk_join_mask(gk_ctx *a, int keep);

/* Screen a batch of reads against the sorted index (no reference routine: the reference offers no
 * search; a window's count is gk_lookup's, by its compare_sba_kmers_lexicographically, kmers.py:306-397).
 * seqs: offsets[nseq] ASCII bytes, host memory, the sequences back to back without separators;
 * sequence j is the bytes [offsets[j], offsets[j + 1]).  offsets: nseq + 1 entries, starting at 0 and
 * never decreasing (empty sequences are allowed); no sequence is longer than 2^32 - 1 bytes.  The bytes
 * are letters of the sba alphabet without '$' (gk_lookup's rule).  K is the sort length.
 * For every window of K bytes that lies inside one sequence, the window's count is exactly what
 * gk_lookup returns as `count` for those K bytes as a query with qlen = K: after GK_SORT_CANONICAL the
 * window stands for min(window, reverse complement).  With GK_SCREEN_BOTH_STRANDS on a forward order
 * the count is count(window) + count(reverse complement of window, the reference's IUPAC complement,
 * sequence_collection.py:402-433), counted once when the window is its own reverse complement; on a
 * canonical order the flag changes nothing.
 * n_present[j] = the number of windows of sequence j with count > 0; occurrences[j] = the sum of the
 * counts of its windows; window_count (may be NULL, else offsets[nseq] entries): entry p = the count of
 * the window that starts at byte p, 0 where none starts (the last K - 1 bytes of a sequence, a sequence
 * shorter than K).  Integer results, the same on every run and on both paths.  A sequence of L bytes
 * has max(0, L - K + 1) windows.  Each byte crosses to the device once; the windows are formed and the
 * per-sequence sums taken there.  Synchronises the stream; leaves the sorted order, the unique view
 * and a join result as they are.
 * GK_E_STATE: no sequence, or not sorted; GK_E_UNSUPPORTED: sort length 0 (None); GK_E_ARG: a null
 * context or array, unknown flag bits, offsets that do not start at 0 or decrease, a sequence over
 * 2^32 - 1 bytes (all checked before any byte of seqs is read); GK_E_ALPHABET: a byte outside the
 * alphabet (found on the device; the message names the sequence, the offset in it and the byte; the
 * outputs are then unspecified).  nseq == 0 returns GK_OK and touches nothing; a total length of 0
 * writes zeros to the per-sequence outputs. */
#define GK_SCREEN_BOTH_STRANDS 1u
int gk_screen(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t flags,
              uint32_t *n_present, uint64_t *occurrences, uint32_t *window_count);

/* The LCP array of the sorted order and what is read off it (no reference routine: the reference
 * answers for one length per call; equality is its compare_sba_kmers_lexicographically, kmers.py:306-397).
 * For a forward (non-canonical) sort and a cap max_len >= 1: lcp[q] (q >= 1) = the largest k in
 * 0..max_len at which sorted k-mers q - 1 and q compare equal at kmer_len = k; lcp[0] = 0, and lcp[n] = 0
 * wherever a successor is needed.  A '$' on both sides at the same offset, after equal bytes, means
 * equal at every length (lcp = max_len); a '$' on one side ends the common prefix.  So for every
 * 1 <= k <= max_len the group head at k is exactly lcp[q] < k, and a k-mer cut short after len bases
 * has lcp in [0, len) or equal to max_len.
 * gk_lcp builds the array as a view of the sorted order (device uint32[*n], like the unique view; dropped
 * by a sort, new starts or a new sequence) or reuses it: a view built for a larger max_len serves a
 * smaller one by clamping, a larger max_len rebuilds it.  After a bounded sort max_len may not exceed
 * the sort length; after a sort with max_kmer_len None it is the caller's choice, and the byte
 * comparison costs up to max_len steps per pair inside long repeats.  Two paths with the same answers:
 * the encoded keys where they decide prefixes (direct keys without a length field: XOR, count leading
 * zeros), else the sequence bytes (bounded variable-length 2-bit keys, rank keys, None, fewer than two
 * k-mers); GKM_LCP_PATH = bytes | keys (gk_set_option) forces one, keys where it does not apply:
 * GK_E_UNSUPPORTED.
 * gk_copy_lcp: entries [offset, offset + count) of the view, clamped to the max_len of the last gk_lcp.
 * gk_device_lcp: the device array; its entries are capped at the cap the view was built with, which is
 * >= the last max_len (a reader clamps).  Both: GK_E_STATE without a valid view.
 * gk_lcp_spectrum: distinct[k] = #{q : lcp[q] < k} (the distinct k-mers of length k) and
 * unique[k] = #{q : max(lcp[q], lcp[q + 1]) < k} (those that occur once), k = 1..max_len, entry 0
 * unused and 0; both arrays hold max_len + 1 entries.  k-mers cut short by a contig end count as
 * gk_group_hist counts them with the keep-all filter.  One pass over the view, built if needed.
 * gk_position_track: a uint32[sba_len] track in sequence order, 0 where no k-mer of the current set
 * starts ('$', contig tails, positions below min_kmer_len, positions outside given starts); sba_len must
 * be the sequence's length; dst may be NULL (the track stays on the device: gk_device_track, the last
 * track built, valid until the next gk_position_track).
 *   GK_TRACK_MIN_UNIQUE    len = the cap: track[starts[q]] = max(lcp[q], lcp[q + 1]) + 1, the shortest
 *                          length at which k-mer q is unique, or GK_NEVER_UNIQUE when that exceeds len.
 *   GK_TRACK_MULTIPLICITY  len = kmer_len (0: the sort length): track[starts[q]] = the size of q's
 *                          group at kmer_len.  At the sort length it also works after GK_SORT_CANONICAL.
 * All synchronise the stream.  GK_E_ARG: a null context or array, max_len == 0 or above 2^24, max_len or
 * kmer_len above the sort length of a bounded sort, an unknown kind, a wrong sba_len; GK_E_STATE: no
 * sequence, or not sorted; GK_E_UNSUPPORTED: a canonical order (no prefixes) for gk_lcp, the
 * spectrum, GK_TRACK_MIN_UNIQUE and a multiplicity at another length than the sort's. */
#define GK_NEVER_UNIQUE 0xFFFFFFFFu
#define GK_TRACK_MIN_UNIQUE 1
#define GK_TRACK_MULTIPLICITY 2
int gk_lcp(gk_ctx *ctx, uint32_t max_len, uint64_t *n);
int gk_copy_lcp(gk_ctx *ctx, uint64_t offset, uint32_t *dst, uint64_t count);
int gk_device_lcp(gk_ctx *ctx, void **lcp, uint64_t *n);
int gk_lcp_spectrum(gk_ctx *ctx, uint32_t max_len, uint64_t *distinct, uint64_t *unique);
int gk_position_track(gk_ctx *ctx, int kind, uint32_t len, uint32_t *dst, uint64_t sba_len);
int gk_device_track(gk_ctx *ctx, void **track, uint64_t *sba_len);

/* Matching statistics of a batch of reads against the sorted index (no reference routine: the reference
 * offers no search; equality and order are gk_lookup's, by its compare_sba_kmers_lexicographically,
 * kmers.py:306-397).  seqs and offsets are gk_screen's batch, with its rules and its checks made before
 * any byte of seqs is read; the bytes are letters of the sba alphabet without '$'.  K is the sort length.
 * The cap C: after a bounded sort max_len is 0 (meaning K) or in 1..K; after a sort with max_kmer_len
 * None it is required and in 1..4096.  Longer matches are reported as C.
 * For byte position p of a sequence that ends at e let m = min(C, e - p).  match_len[p] = the largest l
 * in 0..m for which gk_lookup of the l bytes at p (qlen = l) has count > 0 (presence is monotone in l);
 * match_first[p], match_count[p] = gk_lookup's first and count for that l, both 0 when l = 0.  A match
 * never crosses the end of a read or of a contig; letters compare by byte equality ('N' matches 'N').
 * Each of the three per-position arrays may be NULL (else offsets[nseq] entries): an array that is not
 * asked for costs no device memory and no copy.
 * longest[j] = the maximum of match_len over sequence j's positions, longest_pos[j] = the offset in the
 * sequence of the first position that attains it (0 when longest[j] is 0 or the sequence is empty),
 * sum_len[j] = the sum of match_len.  Integer results, the same on every run and on both paths.
 * Each byte crosses to the device once, in chunks that overlap by C - 1 bytes.  Two paths with the same
 * answers: the sorted one-word 2-bit keys when the context holds them (A/C/G/T-only index, K <= 32,
 * forward order, min_kmer_len == K; a match ends at any other letter of a read), else one search per
 * position over the sorted starts comparing sequence bytes (mixed alphabets, K > 32, k-mers cut short by
 * contig ends, None, rank-key orders); GKM_MATCH_PATH = bytes | keys (gk_set_option) forces one, keys
 * where it does not apply: GK_E_UNSUPPORTED.  GKM_MATCH_CHUNK lowers the bytes of reads per launch.
 * Synchronises the stream; leaves the sorted order, the unique view, a join result and the LCP view as
 * they are.
 * GK_E_STATE: no sequence, or not sorted; GK_E_UNSUPPORTED: a canonical order (no prefixes); GK_E_ARG: a
 * null context or required array, flags != 0 (there are none yet), max_len above K, max_len 0 or above
 * 4096 after None, offsets that do not start at 0 or decrease, a sequence over 2^32 - 1 bytes;
 * GK_E_ALPHABET: a byte outside the alphabet (found on the device; gk_screen's message; the outputs are
 * then unspecified).  Each message names the values.  nseq == 0 returns GK_OK and touches nothing; a
 * total length of 0 writes zeros to the per-sequence outputs. */
int gk_match(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t max_len,
             uint32_t flags, uint32_t *longest, uint32_t *longest_pos, uint64_t *sum_len,
             uint32_t *match_len, uint64_t *match_first, uint32_t *match_count);

/* Minimizer sampling of a batch of reads, or of the loaded sequence (no reference routine; the
 * definition below is the contract).  seqs and offsets are gk_screen's batch; the offsets are checked by
 * gk_screen's rules before any byte of seqs is read.  k is in 1..32, w in 1..256.
 *   valid start  byte position p is a valid start if p + k <= the end of its sequence and its k bytes
 *                are all 'A', 'C', 'G' or 'T'.  Any other byte -- '$', 'N', an IUPAC letter, a byte
 *                outside the alphabet -- only ends a run: there is no alphabet error in these calls.
 *   key(p)       the k bases as the 2-bit key in the low 2 k bits: A 0, C 1, G 2, T 3, the first base
 *                most significant.  With GK_MINIMIZER_CANONICAL ckey = min(key, revcomp(key)) and
 *                strand = 1 iff revcomp(key) < key (a k-mer equal to its reverse complement has strand
 *                0); without the flag ckey = key and strand = 0.
 *   ord(p)       with GK_MINIMIZER_LEX ord = ckey; otherwise ord = mix(ckey), mix(x) =
 *                fmix64(x ^ 0x9E3779B97F4A7C15), fmix64(h): h ^= h >> 33; h *= 0xff51afd7ed558ccd;
 *                h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53; h ^= h >> 33, all mod 2^64.  mix is a bijection,
 *                so equal ords mean equal k-mers; the XOR keeps poly-A from hashing to 0.  ords compare
 *                as unsigned 64-bit numbers.
 *   window       w consecutive positions s .. s + w - 1 that are all valid starts of the same sequence
 *                (at k = 1 consecutive valid starts can straddle two sequences: no window there).
 *   minimizer    a window's minimizer is its leftmost position of least ord.
 * The result is the set of positions that are the minimizer of at least one window, ascending, each
 * with its ckey and strand; per sequence, the number of its positions in the set.  A run of fewer than
 * w valid starts selects nothing; w = 1 selects every valid start.  The same set by a local rule: p is
 * selected iff p is valid and L(p) + R(p) + 1 >= w, L(p) = the consecutive valid left neighbours in the
 * same sequence with ord > ord(p), R(p) = the consecutive valid right neighbours with ord >= ord(p),
 * both capped at w - 1.
 * gk_minimizers needs a context, but no loaded sequence and no sort.  Each byte crosses to the device
 * once, in chunks: a chunk owns a range of positions and carries w - 1 more bytes on its left and
 * w - 1 + k - 1 on its right (fewer at the batch's ends); GKM_MINIMIZER_CHUNK (gk_set_option) lowers
 * the positions a chunk owns.  The result stays on the device as a view -- pos uint64 (byte positions
 * in the batch), key uint64, strand uint8, *n_out entries each -- until the next gk_minimizers or
 * gk_destroy; the call touches no sort state, unique view, join result or LCP view.  per_seq (may be
 * NULL, else nseq entries): the count of each sequence.  Integer results, the same on every run and for
 * every chunk size.  nseq == 0 returns GK_OK with *n_out = 0 (an empty view).  A call refused with
 * GK_E_ARG has touched nothing, an earlier view included; any other failure leaves no view.
 * gk_copy_minimizers copies the view (each array may be NULL; n must equal the view's count, else
 * GK_E_ARG); gk_device_minimizers gives the device arrays.  Both: GK_E_STATE without a view.
 * gk_select_minimizers applies the same selection to the loaded sequence taken as one sequence (its '$'
 * separators are invalid bytes, so no window crosses a contig end) and installs the selected positions,
 * ascending, as the context's start set: the state gk_set_start_indices(ctx, those positions, n, k)
 * would leave (min_kmer_len = k; the sort state, every view and a prefetched first pass dropped), the
 * positions never visiting the host.  n_out may be NULL.  GK_E_STATE without a sequence; a call refused
 * with GK_E_ARG or GK_E_STATE has touched nothing, a prefetched first pass included.
 * All synchronise the stream.  GK_E_ARG: a null context, a null required pointer (offsets, n_out of
 * gk_minimizers, seqs of a batch with bytes), k outside 1..32, w outside 1..256, unknown flag bits,
 * offsets that break gk_screen's rules.  Each message names the values. */
#define GK_MINIMIZER_CANONICAL 1u
#define GK_MINIMIZER_LEX       2u
int gk_minimizers(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq,
                  uint32_t k, uint32_t w, uint32_t flags, uint64_t *n_out, uint32_t *per_seq);
int gk_copy_minimizers(gk_ctx *ctx, uint64_t *pos, uint64_t *key, uint8_t *strand, uint64_t n);
int gk_device_minimizers(gk_ctx *ctx, void **pos, void **key, void **strand, uint64_t *n);
int gk_select_minimizers(gk_ctx *ctx, uint32_t k, uint32_t w, uint32_t flags, uint64_t *n_out);

/* ---- FASTA ingest (host; no context, no device) ------------------------------------------
 * gk_fasta_open maps `path` and scans it once with n_threads threads (<= 0: up to 16): the
 * number of records ('>' lines), the sequence bytes left after each line's strip(), and the bytes
 * of the record names (each NUL-terminated) -- _get_fasta_stats (sequence_collection.py:476-515).
 * The caller allocates sba[total_seq_len + num_records - 1], seg_starts[num_records] and
 * names[names_bytes]; gk_fasta_fill writes them as _load_forward_sba_from_fasta does (:517-566):
 * upper-cased bytes, '$' between records, segment starts, names in record order.  bad_bytes[256]
 * (optional, zeroed by the caller) flags every sequence byte outside ACGTRYSWKMBDHVN$, for the
 * reference's alphabet error (:571-574).  GK_E_FASTA_NAME: a header without a name;
 * GK_E_FASTA_LAYOUT: the bytes do not fill sba exactly.  gk_fasta_close unmaps. */
int gk_fasta_open(const char *path, int n_threads, gk_fasta **out, uint64_t *num_records, uint64_t *total_seq_len,
                  uint64_t *names_bytes);
int gk_fasta_fill(gk_fasta *f, uint8_t *sba, uint64_t sba_len, uint32_t *seg_starts, char *names,
                  uint8_t *bad_bytes);
void gk_fasta_close(gk_fasta *f);

/* ---- synthetic genomes (host) --------------------------------------------------------------
 * The reference's profiling genome: profiling.get_random_seq(n) after np.random.seed(seed)
 * (profiling.py:12-24) -- MT19937 init_genrand(seed), base i = "ATGC"[genrand_int32() & 3] --
 * written as n ASCII bytes. */
int gk_reference_random_bases(uint8_t *out, uint64_t n, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* GKM_H */
