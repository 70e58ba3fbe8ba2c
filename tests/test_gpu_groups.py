"""The group pass (gkm_group.hip: group_front, gk_group_hist, gk_group_members; gk_locate at the
C boundary, gkm_capi.hip) past one 4,096-flag scan tile: prefix groups on the keys and on the bytes, built-in
filters on the per-position and the per-k-mer path, histogram bins around the LDS split, yields
with groups larger than a tile, head masks, the chunked tile-sum scan and every grid-stride loop
past its grid cap.

Every integer output is compared bit-exact with tests/groupref.py (pinned by tests/test_groupref.py
against the golden vectors and the C oracle) on the device's own current order -- the order itself
is checked by the sort's tests.  Every test first proves its premise from the reference alone: the
group sizes it is about occur in the reference histogram, the filter fails the wanted k-mers, the
path condition (n * 8 against sba_len) holds.
"""

import numpy as np
import pytest

import groupref
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection
from oracle import oracle

pytestmark = pytest.mark.gpu

TILE = 4096  # kScanTile (gkm_internal.h): flags per scan tile
KEEP = (groupref.KEEP_ALL, 0, 0, 0)
MASK = (_native.FILTER_MASK, 0, 0, 0)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# one device query against the reference
# ---------------------------------------------------------------------------------------------
def make_engine(sba, min_k, sort_len="unsorted", starts=None):
    """An engine over sba with the enumerated (or the given) starts, sorted at sort_len (None: the
    suffix order) unless "unsorted"; -> (engine, the device's current order)."""
    e = _native.Engine()
    e.set_sequence(sba, groupref.segments_of(sba))
    if starts is None:
        e.enumerate(min_k)
    else:
        e.set_start_indices(starts, min_k)
    if sort_len != "unsorted":
        e.sort(sort_len)
    return e, e.copy_starts()


def device_query(e, is_sorted, kmer_len, filt, kw):
    f = _native.GkFilter(filt[0], 0, filt[1], filt[2], filt[3])
    lo, hi = kw.get("min_group_size", 1), kw.get("max_group_size")
    try:
        if "max_counts_bin" in kw:
            return "ok", e.group_hist(is_sorted, kmer_len, f, lo, hi, kw["max_counts_bin"])
        return "ok", e.group_members(is_sorted, kmer_len, f, lo, hi, kw.get("yield_first_n"))
    except _native.FilterRaised as ex:
        return "raise", ex.sba_idx, ex.ferr


def reference_query(sba, st, is_sorted, kmer_len, filt, kw, mask=None, heads=None):
    if filt[0] == _native.FILTER_MASK:
        return "ok", groupref.group_scan(sba, st, kmer_len, valid=mask, is_sorted=bool(is_sorted), heads=heads, **kw)
    if heads is not None:
        return "ok", groupref.group_scan(sba, st, kmer_len, heads=heads, **kw)
    return groupref.scan_filtered(sba, st, kmer_len, filt, is_sorted=bool(is_sorted), **kw)


def assert_same(got, want, ctx):
    assert got[0] == want[0], (ctx, got if got[0] == "raise" else None, want if want[0] == "raise" else None)
    if got[0] == "raise":
        assert got[1:] == want[1:], ctx  # (sba index, gk_filter_error) of the first raise
    elif isinstance(want[1][1], int):
        np.testing.assert_array_equal(got[1][0], want[1][0], err_msg=str(ctx))
        assert got[1][1] == want[1][1], ctx
    else:
        for g, w in zip(got[1], want[1]):
            assert g.dtype == w.dtype and g.shape == w.shape, ctx
            np.testing.assert_array_equal(g, w, err_msg=str(ctx))


def check(e, sba, st, kmer_len, filt=KEEP, is_sorted=True, mask=None, heads=None, **kw):
    """One device query == the reference on the order st; -> the reference's answer."""
    want = reference_query(sba, st, is_sorted, kmer_len, filt, kw, mask, heads)
    got = device_query(e, _native.GROUPS_FROM_HEADS if heads is not None else is_sorted, kmer_len, filt, kw)
    assert_same(got, want, (kmer_len, filt, is_sorted, kw))
    return want


HIST = dict(max_counts_bin=64)
PAIRS = dict(min_group_size=2, yield_first_n=2)


def check_hist_and_pairs(e, sba, st, kmer_len, filt=KEEP, **extra):
    """Histogram + the first two members of every group of two or more; the reference must have
    such groups (else the yields are empty and the case checks nothing)."""
    want = check(e, sba, st, kmer_len, filt, **HIST, **extra)
    assert want[1][0][2:].sum() > 0, ("no group of two or more k-mers in the reference", kmer_len, filt)
    want = check(e, sba, st, kmer_len, filt, **PAIRS, **extra)
    assert len(want[1][0]) > 0
    return want


def fails_some(sba, st, filt):
    """premise of a filtered case: the filter raises nowhere, fails some k-mers and passes some"""
    passes, err = groupref.filter_eval(sba, st, *filt)
    assert not err.any() and 0 < passes.sum() < len(st), (filt, int(passes.sum()), len(st))
    return passes


def flip_code_bit(bases, bit, four_bit):
    """the letters whose key codes (oracle.CODE2 / CODE4) differ from the given ones in one bit;
    a letter without such a partner (the code would be 0, the 4-bit '$') stays"""
    order = oracle.CODE4_ORDER if four_bit else b"ACGT"
    first = 1 if four_bit else 0
    table = np.arange(256, dtype=np.uint8)
    for i, c in enumerate(order):
        code = (i + first) ^ bit
        if first <= code < first + len(order):
            table[c] = order[code - first]
    return table[bases]


def random_contigs(rng, lengths, alphabet=b"ACGT", repeat_len=900, copies=4, n_runs=0):
    """contigs of the given lengths joined by '$', a repeat planted `copies` times (so groups exist
    at every k-mer length up to repeat_len) and twice more with a substitution every 131 bases: in
    one copy by the letter whose key code differs in the lowest bit, in the other in the highest (so
    k-mers agree on a prefix of every length up to 130 and differ by one key bit right after it);
    n_runs runs of 40-200 N"""
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    four_bit = alphabet != b"ACGT" or n_runs > 0
    rep = rng.choice(letters, repeat_len).astype(np.uint8)
    parts = []
    for L in lengths:
        c = rng.choice(letters, L).astype(np.uint8)
        if L > 2 * repeat_len:
            for copy in range(copies + 2):
                at = int(rng.integers(0, L - repeat_len))
                c[at:at + repeat_len] = rep
                if copy >= copies:
                    sites = np.arange(int(rng.integers(100, 131)), repeat_len, 131)
                    bit = 1 if copy == copies else (8 if four_bit else 2)
                    c[at + sites] = flip_code_bit(rep[sites], bit, four_bit)
        elif L > 40:  # a short contig: a piece of the repeat
            c[:] = rep[:L]
        if L > 40:  # every contig ends alike, so k-mers that end at '$' before kmer_len meet in groups
            c[-20:] = rep[-20:]
        for _ in range(n_runs if L > 2000 else 0):
            at = int(rng.integers(0, L - 200))
            c[at:at + int(rng.integers(40, 200))] = ord("N")
        parts += [c, np.array([groupref.DOLLAR], dtype=np.uint8)]
    return np.concatenate(parts[:-1])


def small_n(n):
    assert 2 * TILE < n < 4 * TILE and n % 16 != 0, n


# ---------------------------------------------------------------------------------------------
# prefix groups on the keys: head_flags_kernel<0, W>, with and without a compaction index
# ---------------------------------------------------------------------------------------------
KEY_CASES = [
    ("acgt-k31", b"ACGT", 31, [1, 16, 30, 31], 0),
    ("acgt-k40", b"ACGT", 40, [8, 32, 33, 39, 40], 0),
    ("acgt-k63", b"ACGT", 63, [32, 62, 63], 0),
    ("acgt-k64", b"ACGT", 64, [32, 63, 64], 0),
    ("acgt-k100", b"ACGT", 100, [32, 64, 96, 99], 0),
    ("iupac-k31", b"ACGTACGTACGTNRYKMSWBDHV", 31, [15, 16, 17, 30, 31], 0),
    ("mixed-n-runs-k31", b"ACGT", 31, [16, 31], 6),
]
HOMO16 = (groupref.HOMOPOLYMER, 3, 16, 0)
ALL_PASS = (groupref.LENGTH, 1, 0, 0)


def differ_in_top_bits(keys, total_bits, nbits):
    """out[q - 1] = keys q - 1 and q (rows of uint64 words, most significant first, total_bits used)
    differ somewhere in their top nbits"""
    words = keys.shape[1]
    out = np.zeros(len(keys) - 1, dtype=bool)
    for w in range(words):
        low = (words - 1 - w) * 64  # bit index of the word's bit 0
        mask = sum(1 << b for b in range(64) if total_bits - nbits <= low + b < total_bits)
        out |= ((keys[1:, w] ^ keys[:-1, w]) & np.uint64(mask)) != 0
    return out


@pytest.mark.parametrize("name,alphabet,K,kmer_lens,n_runs", KEY_CASES, ids=[c[0] for c in KEY_CASES])
def test_prefix_groups_on_keys(name, alphabet, K, kmer_lens, n_runs):
    """kmer_len below the sort length K: the masked key compare, for 1 to 4 key words, 2-bit and
    4-bit keys, prefixes that end on or straddle a 64-bit word; each with keep-all and behind a
    homopolymer filter (the heads then compare cidx[q - 1] with cidx[q]).  At kmer_len == K the
    keep-all query takes the heads the sort wrote (no group_heads timer); the same query behind an
    all-pass filter recomputes them (the timer runs) and must give the same output.  Premise, from
    the reference and the oracle's key encoding: at every queried length neighbours of the sorted
    order differ in the last compared key bit only and in the first bit after it only, so a key
    mask that is one bit too short or too long gives other heads."""
    rng = np.random.default_rng(100 + K + len(alphabet))
    sba = random_contigs(rng, [10_007 + K], alphabet=alphabet, n_runs=n_runs)
    e, st = make_engine(sba, K, K)
    small_n(len(st))
    words, bits, symbols = e.key_layout()
    assert symbols == K and bits == (2 if alphabet == b"ACGT" and not n_runs else 4)
    assert words == (K * bits + 63) // 64
    fails_some(sba, st, HOMO16)
    keys = oracle.encode_keys(sba, st, bits, K, 0, words)
    groups = {k: groupref.group_scan(sba, st, k, max_counts_bin=1)[0].sum()
              for q in kmer_lens for k in (q - 1, q, q + 1) if 1 <= k <= K}
    for kmer_len in kmer_lens:
        # some neighbours agree on kmer_len - 1 symbols and differ in the last, others agree on
        # kmer_len and differ in the next: a key mask one symbol (or one bit of it) off moves a head
        assert groups.get(kmer_len - 1, 0) < groups[kmer_len] < groups.get(kmer_len + 1, len(st) + 1), kmer_len
        if kmer_len < K:  # the same in bits of the key: one bit more or fewer in the mask moves a head
            heads = differ_in_top_bits(keys, bits * K, bits * kmer_len)
            assert heads.sum() + 1 == groups[kmer_len]
            assert (heads != differ_in_top_bits(keys, bits * K, bits * kmer_len - 1)).any(), kmer_len
            assert (heads != differ_in_top_bits(keys, bits * K, bits * kmer_len + 1)).any(), kmer_len
        check_hist_and_pairs(e, sba, st, kmer_len)
        check_hist_and_pairs(e, sba, st, kmer_len, HOMO16)
    if K in kmer_lens:
        e.profile_enable(True)
        direct = device_query(e, 1, K, KEEP, PAIRS), device_query(e, 1, K, KEEP, HIST)
        assert "group_heads" not in e.profile_report(), "keep-all at the sort length must reuse the sort's heads"
        e.profile_enable(True)
        recomputed = device_query(e, 1, K, ALL_PASS, PAIRS), device_query(e, 1, K, ALL_PASS, HIST)
        assert e.profile_report()["group_heads"]["count"] == 3  # the yields take two calls (count, then fill)
        e.profile_enable(False)
        assert groupref.filter_eval(sba, st, *ALL_PASS)[0].all()
        for a, b in zip(direct, recomputed):
            assert_same(a, b, (name, "sort-written heads against recomputed heads"))


# ---------------------------------------------------------------------------------------------
# byte-compare groups: head_flags_kernel<1, 1> / sba_equal
# ---------------------------------------------------------------------------------------------
BYTE_CASES = [  # (id, min, sort length, query lengths)
    ("bounded-5-12", 5, 12, [3, 5, 8, 12]),
    ("suffix", 5, None, [None, 7]),
    ("fixed-20", 20, 20, [25, 60]),
]


@pytest.mark.parametrize("name,min_k,sort_len,kmer_lens", BYTE_CASES, ids=[c[0] for c in BYTE_CASES])
def test_byte_compare_groups(name, min_k, sort_len, kmer_lens):
    """Variable-length keys with a length field queried below their length, rank keys at another
    length, and kmer_len above the sort length: k-mers that end at a '$' (or the end of the sba)
    before kmer_len are equal only to k-mers that end after as many equal bases (every contig of
    more than 40 bases ends in the same 20, so such k-mers meet in groups)."""
    rng = np.random.default_rng(200 + min_k)
    lengths = [3000, min_k, 2500, 37, 1999, 2806]  # ragged, one contig of exactly min_k bases
    sba = random_contigs(rng, lengths, repeat_len=300, copies=3)
    e, st = make_engine(sba, min_k, sort_len)
    small_n(len(st))
    filt = (groupref.HOMOPOLYMER, 2, min_k, 0)
    fails_some(sba, st, filt)
    nd = groupref.bases_before_end(sba)[st]
    for kmer_len in kmer_lens:
        if kmer_len is None or kmer_len > min_k:
            short = nd < (kmer_len or 1 << 30)
            assert short.sum() > len(lengths), "k-mers must end at '$' before kmer_len"
        want = check_hist_and_pairs(e, sba, st, kmer_len)
        check_hist_and_pairs(e, sba, st, kmer_len, filt)
        if kmer_len is None or kmer_len > min_k:
            # some group of two or more holds a k-mer that ends before kmer_len
            assert (nd[want[1][0].astype(np.int64)] < (kmer_len or 1 << 30)).any()
        check(e, sba, st, kmer_len)  # every member of every group


# ---------------------------------------------------------------------------------------------
# big groups: planted exact multiplicities around the histogram's LDS split and above one tile
# ---------------------------------------------------------------------------------------------
PLANTED = (2047, 2048, 2049, 5000)
HOMOPOLYMER_GROUP = 10_000
GC31 = (groupref.GC, 11, 18, 31)


def _planted_31mer(rng, gc):
    u = np.where(np.arange(31) < gc, ord("G"), ord("A")).astype(np.uint8)
    u[:gc:2] = ord("C")
    u[gc::2] = ord("T")
    return rng.permutation(u)


@pytest.fixture(scope="module")
def big_groups():
    """~410 k bases: four random 31-mers (G/C counts 14, 15, 16: they pass GC31) in exactly 2047,
    2048, 2049 and 5000 copies, each copy followed by two varying bases; a homopolymer that gives
    one group of 10,000 31-mers; 40 k random bases (more than 4,096 groups) with a 200-base
    segment in three copies.  -> (sba, engine sorted
    at 31, order, reference sizes of all groups at 31)"""
    rng = np.random.default_rng(31)
    parts = [ACGT[rng.integers(0, 4, 20_000)]]
    for mult, gc in zip(PLANTED, (14, 15, 16, 15)):
        u = _planted_31mer(rng, gc)
        block = np.empty((mult, 33), dtype=np.uint8)
        block[:, :31] = u
        block[:, 31:] = ACGT[rng.integers(0, 4, (mult, 2))]
        parts.append(block.ravel())
    tail = ACGT[rng.integers(0, 4, 20_000)]
    tail[5000:5200] = tail[9000:9200] = tail[:200]  # groups of three
    parts.append(tail)
    parts.append(np.full(HOMOPOLYMER_GROUP + 30, ord("A"), dtype=np.uint8))
    parts.append(ACGT[rng.integers(1, 4, 7)])
    sba = np.concatenate(parts)
    e, st = make_engine(sba, 31, 31)
    hist, total = groupref.group_scan(sba, st, 31, max_counts_bin=1_000_000)
    assert total == len(st) and len(st) % 16 != 0
    for size in PLANTED + (HOMOPOLYMER_GROUP,):
        assert hist[size] == 1, (size, "planted multiplicity missing from the reference histogram")
    assert hist.sum() > TILE, "more groups than one scan tile"
    return sba, e, st, hist


def test_query_sequence_on_one_context(big_groups):
    """A filtered query overwrites the context's flags and group starts; the unfiltered queries and
    gk_unique_counts after it must not see any of that."""
    sba, e, st, ref_hist = big_groups
    n = len(st)
    sizes = np.repeat(np.arange(len(ref_hist)), ref_hist)  # the group sizes, ascending
    first = check(e, sba, st, 31, max_counts_bin=6000)
    passes = fails_some(sba, st, GC31)
    want = check(e, sba, st, 31, GC31, min_group_size=2, yield_first_n=3)
    assert want[1][2].max() >= 5000 and (want[1][0] != np.arange(len(want[1][0]))).any()
    again = device_query(e, 1, 31, KEEP, dict(max_counts_bin=6000))
    assert_same(again, first, "keep-all after a filtered query")
    assert_same(again, ("ok", (np.bincount(np.minimum(sizes, 6000), minlength=6001), n)), "reference sizes")

    def unique_matches():
        num, _, tot = groupref.group_scan(sba, st, 31, yield_first_n=1)
        starts, counts = e.unique_counts()
        np.testing.assert_array_equal(starts, num)
        np.testing.assert_array_equal(counts, tot)
        np.testing.assert_array_equal(np.bincount(np.minimum(counts, 6000), minlength=6001), again[1][0])

    unique_matches()
    mask = (np.random.default_rng(7).random(n) < 0.5).astype(np.uint8)
    assert 0 < mask.sum() < n and not np.array_equal(mask.astype(bool), passes)
    e.set_filter_mask(mask)
    check(e, sba, st, 31, MASK, mask=mask, max_counts_bin=6000)
    check(e, sba, st, 31, MASK, mask=mask, min_group_size=2, yield_first_n=3)
    unique_matches()
    assert_same(device_query(e, 1, 31, KEEP, dict(max_counts_bin=6000)), first, "keep-all after a mask query")


BIN_SELECTIONS = [dict(), dict(min_group_size=2048), dict(max_group_size=2048)]


@pytest.mark.parametrize("max_counts_bin", [1, 2, 2047, 2048, 2049, 6000, 1_000_000])
def test_histogram_bins(big_groups, max_counts_bin):
    """group_hist_kernel keeps bins below 2,048 in LDS and adds the others to global memory; sizes
    above max_counts_bin land in the last bin.  Groups of 2047, 2048, 2049, 5000 and 10,000 members
    against bin limits on both sides of the split, with the size selections on both sides too."""
    sba, e, st, ref_hist = big_groups
    for sel in BIN_SELECTIONS:
        want = check(e, sba, st, 31, max_counts_bin=max_counts_bin, **sel)
        hist = want[1][0]
        if max_counts_bin >= HOMOPOLYMER_GROUP:
            on = [s for s in PLANTED + (HOMOPOLYMER_GROUP,)
                  if s >= sel.get("min_group_size", 1) and s <= sel.get("max_group_size", 1 << 30)]
            assert all(hist[s] == 1 for s in on) and len(on) >= 2
        elif "max_group_size" not in sel:  # 6000: the 10,000 alone; below: several sizes share the overflow bin
            assert hist[max_counts_bin] >= (1 if max_counts_bin == 6000 else 2)


def test_kmer_count_through_kmers(big_groups):
    """Kmers.get_kmer_count always asks for 1,000,000 bins; get_kmer_group_counts for the caller's."""
    sba, _, _, _ = big_groups
    sc = SequenceCollection(sequence_list=[("c0", sba.tobytes().decode())])
    km = gk.Kmers(sc, min_kmer_len=31, max_kmer_len=31)
    km.sort()
    st = km.kmer_sba_start_indices
    for sel in BIN_SELECTIONS:
        _, total = groupref.group_scan(sba, st, 31, max_counts_bin=10, **sel)
        assert 0 < total and km.get_kmer_count(31, **sel) == total
    _, total = groupref.scan_filtered(sba, st, 31, GC31, max_counts_bin=10, min_group_size=2048)[1]
    filt = gk.gen_kmer_gc_content_filter_func(0.35, 0.6, 31)
    assert filt.params == GC31[1:]
    assert total >= 2048 and km.get_kmer_count(31, filt, min_group_size=2048) == total
    hist, total = km.get_kmer_group_counts(31, filt, max_counts_bin=2048)
    want = groupref.scan_filtered(sba, st, 31, GC31, max_counts_bin=2048)[1]
    np.testing.assert_array_equal(hist, want[0])
    assert total == want[1]


@pytest.mark.parametrize("filt", [KEEP, GC31], ids=["keep-all", "gc"])
@pytest.mark.parametrize("yield_first_n", [1, 3, None])
def test_yields_past_one_tile(big_groups, filt, yield_first_n):
    """group_yield_count_kernel, the u32 scan and group_yield_write_kernel with more than 4,096
    groups, groups larger than a tile (tiles of the group scan without a head) and, behind the
    filter, kmer_num mapped back through the compaction index."""
    sba, e, st, _ = big_groups
    valid = None
    if filt != KEEP:
        valid = fails_some(sba, st, filt)
    hist, _ = groupref.group_scan(sba, st, 31, valid=valid, max_counts_bin=20_000)
    assert hist.sum() > TILE and hist[TILE + 1:].sum() >= 1 and hist[2048:5001].sum() >= 3 and hist[2:6].sum() >= 1
    assert hist[2 * TILE:].sum() == (valid is None), "keep-all: a group that leaves whole tiles without a head"
    for lo, hi in [(1, None), (2, None), (2, 5), (2048, 5000), (10_000, None)]:
        want = check(e, sba, st, 31, filt, min_group_size=lo, max_group_size=hi, yield_first_n=yield_first_n)
        # (the homopolymer's 10,000 k-mers hold no G/C: behind the GC filter that selection is empty)
        assert (len(want[1][0]) > 0) != (valid is not None and lo == 10_000), (lo, hi)
        if valid is not None and lo <= 2:
            assert not valid[:int(want[1][0].max())].all(), "kmer_num must differ from the compacted index"
    nothing = check(e, sba, st, 31, filt, min_group_size=20_000, yield_first_n=yield_first_n)
    assert len(nothing[1][0]) == 0


# ---------------------------------------------------------------------------------------------
# tiny and tile-edge sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 4097])
def test_sizes_around_a_vector_and_a_tile(n):
    rng = np.random.default_rng(n)
    sba = ACGT[rng.integers(0, 4, n + 7)].copy()
    sba[3:6] = ord("A")  # a homopolymer of three
    if n >= 15:
        sba[n // 2 + 4:n // 2 + 7] = sba[:3]  # a repeated 3-mer where there is room
    e, st = make_engine(sba, 8, 8)
    assert len(st) == n
    filt = (groupref.HOMOPOLYMER, 2, 8, 0)
    passes, err = groupref.filter_eval(sba, st, *filt)
    assert not err.any() and (n == 1 or 0 < passes.sum() < n)
    for kmer_len in (3, 8):
        check(e, sba, st, kmer_len, **HIST)
        check(e, sba, st, kmer_len)
        check(e, sba, st, kmer_len, filt, **HIST)
        check(e, sba, st, kmer_len, filt, yield_first_n=1)


# ---------------------------------------------------------------------------------------------
# built-in filters: the per-position path (filter_pos_kernel + filter_gather_kernel)
# ---------------------------------------------------------------------------------------------
EDGE_IDS = [f"sba{e[0]}-k{e[2]}" for e in groupref.EDGE_INPUTS]
SELECT23 = dict(max_counts_bin=3, min_group_size=2, max_group_size=5)


def _edge_input(sba_len, contigs, K, n_run):
    sba = groupref.iupac_sequence(sba_len, contigs, seed=sba_len, n_run=n_run)
    assert len(sba) == sba_len
    return sba


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("sba_len,contigs,K,n_run", groupref.EDGE_INPUTS, ids=EDGE_IDS)
def test_builtin_filters_per_position(sba_len, contigs, K, n_run, sort):
    """Every built-in kind at ordinary and edge parameters on sequences whose length is 1 and 33
    past a multiple of 64 (and 40, 63: less than one wave of positions), k-mers up to the last
    position that can start one: histogram, total, yields, or the code and sba index of the first
    raise in the current order."""
    sba = _edge_input(sba_len, contigs, K, n_run)
    e, st = make_engine(sba, K, K if sort else "unsorted")
    n = len(st)
    assert n * 8 >= sba_len, "per-position path"
    if sba_len > 64:
        small_n(n)
        assert {0, 31, 32, 63} <= set((st % 64).tolist()) and st.max() == sba_len - K
    outcomes = {}
    for label, filt in groupref.filter_cases(K):
        want = check(e, sba, st, K, filt, is_sorted=sort, **HIST)
        check(e, sba, st, K, filt, is_sorted=sort, **SELECT23)
        check(e, sba, st, K, filt, is_sorted=sort, **PAIRS)
        check(e, sba, st, K, filt, is_sorted=sort)
        outcomes[label] = want
    raised = {label: w[2] for label, w in outcomes.items() if w[0] == "raise"}
    assert {"homopolymer-raises", "gc-raises", "no-ambiguous-raises", "homopolymer-len-below-max-past-end"} \
        <= set(raised)
    assert raised["homopolymer-len-below-max-past-end"] == groupref.FERR_HOMO_LEN
    for label in ("gc-empty-window", "homopolymer-len-below-max", "length-1-all-pass"):
        assert outcomes[label][0] == "ok", label
    assert outcomes["gc-empty-window"][1][1] == 0 and outcomes["length-1-all-pass"][1][1] == n
    assert outcomes["homopolymer-len-below-max"][1][1] == n
    if sba_len > 64:
        assert 0 < outcomes["gc-exact-count"][1][1] < n
        assert outcomes["crispr-ngg"][0] == "ok" and 0 < outcomes["crispr-ngg"][1][1] < n
    else:
        assert raised["crispr-ngg"] == groupref.FERR_CRISPR_LEN


@pytest.mark.parametrize("sba_len,contigs,K,n_run", groupref.EDGE_INPUTS[:2], ids=EDGE_IDS[:2])
def test_crispr_reads_across_a_separator_and_raises_at_the_end(sba_len, contigs, K, n_run):
    """crispr_ngg_pam_filter looks at sba[idx + 21] and sba[idx + 22] whatever lies between: a guide
    that crosses a '$' in the middle of the sba is answered, one in the last 22 positions raises."""
    sba = _edge_input(sba_len, contigs, K, n_run)
    crispr = (groupref.CRISPR_NGG, 0, 0, 0)
    every = groupref.enumerate_starts(sba, 8)
    e, st = make_engine(sba, 8, 8, starts=every)
    assert len(st) * 8 >= sba_len
    want = check(e, sba, st, 8, crispr, **HIST)
    assert want[0] == "raise" and want[2] == groupref.FERR_CRISPR_LEN and want[1] + 23 > sba_len
    inner = groupref.crispr_safe_starts(sba, every)
    e, st = make_engine(sba, 8, 8, starts=inner)
    assert len(st) * 8 >= sba_len
    nd = groupref.bases_before_end(sba)[st]
    passes, err = groupref.filter_eval(sba, st, *crispr)
    assert not err.any() and (passes & (nd < 23)).any() and (~passes & (nd < 23)).any(), \
        "guides that cross a '$' must pass and fail"
    check_hist_and_pairs(e, sba, st, 8, crispr)


FERR_MESSAGES = {
    groupref.FERR_HOMO_LEN: (ValueError, "The kmer_len ({k}) requested is too large for kmer_sba_start_idx ({idx})"),
    groupref.FERR_GC_LEN: (ValueError, "The kmer_len ({k}) requested is too larger for kmer_sba_start_idx ({idx})"),
    groupref.FERR_GC_OOB: (IndexError, "kmer at sba index {idx} of length {k} extends beyond len(sba)"),
    groupref.FERR_AMBIG_LEN: (ValueError, "kmer_len ({k}) is invalid. It extends beyond len(sba)"),
    groupref.FERR_AMBIG_SEG: (ValueError, "end of segment was reached. kmer_len ({k}) invalid."),
    groupref.FERR_CRISPR_LEN: (ValueError, "The guide defined at this start index extends beyond the sba"),
}


@pytest.mark.parametrize("code,one_contig,make,k", [
    (groupref.FERR_HOMO_LEN, False, lambda: gk.gen_kmer_homopolymer_filter_func(3, 14), 14),
    (groupref.FERR_GC_LEN, False, lambda: gk.gen_kmer_gc_content_filter_func(0.0, 1.0, 14), 14),
    (groupref.FERR_GC_OOB, True, lambda: gk.gen_kmer_gc_content_filter_func(0.0, 1.0, 14), 14),
    (groupref.FERR_AMBIG_LEN, True, lambda: gk.gen_no_ambiguous_bases_filter(14), 14),
    (groupref.FERR_AMBIG_SEG, False, lambda: gk.gen_no_ambiguous_bases_filter(14), 14),
    (groupref.FERR_CRISPR_LEN, True, lambda: gk.crispr_ngg_pam_filter, None),
], ids=["homo_len", "gc_len", "gc_oob", "ambig_len", "ambig_seg", "crispr_len"])
def test_filter_errors_through_kmers(code, one_contig, make, k):
    """Each gk_filter_error as the exception the reference raises, type and message, through the
    unsorted Kmers (first raise = first in position order: at the first '$', or -- one contig, where
    a GC window runs off the sba without meeting a '$' -- at the end)."""
    rng = np.random.default_rng(9)
    seqs = [("c0", ACGT[rng.integers(0, 4, 40)].tobytes().decode())]
    if not one_contig:
        seqs.append(("c1", ACGT[rng.integers(0, 4, 52)].tobytes().decode()))
    sc = SequenceCollection(sequence_list=seqs)
    km = gk.Kmers(sc, min_kmer_len=8, max_kmer_len=8)
    filt = make()
    st = km.kmer_sba_start_indices
    assert len(st) * 8 >= len(sc.forward_sba)
    idx, ref_code = groupref.first_raise(st, groupref.filter_eval(sc.forward_sba, st, filt.kind, *filt.params)[1])
    assert ref_code == code
    exc_type, message = FERR_MESSAGES[code]
    with pytest.raises(exc_type) as got:
        km.get_kmer_count(8, filt)
    assert type(got.value) is exc_type and str(got.value) == message.format(k=k, idx=idx)
    with pytest.raises(exc_type) as got:
        list(km.get_kmers(8, kmer_filter_func=filt))
    assert str(got.value) == message.format(k=k, idx=idx)


# ---------------------------------------------------------------------------------------------
# built-in filters: the per-k-mer path (filter_flags_kernel) for a small assigned start set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sba_len,contigs,K,n_run", groupref.EDGE_INPUTS[:2], ids=EDGE_IDS[:2])
def test_builtin_filters_per_kmer(sba_len, contigs, K, n_run):
    """n * 8 < sba_len sends every built-in filter through filter_flags_kernel: 1 in 16 of the valid
    starts plus the starts at word offsets 0, 31, 32, 63 and the last valid one, with duplicates,
    assigned shuffled and then sorted.  Against the reference, and -- where the filter raises
    nowhere -- against the per-position path's pass / fail answer for the same starts."""
    sba = _edge_input(sba_len, contigs, K, n_run)
    every = groupref.enumerate_starts(sba, K)
    rng = np.random.default_rng(sba_len)
    edge = np.concatenate([every[every % 64 == r][:3] for r in (0, 31, 32, 63)] + [every[-1:]])
    pick = np.concatenate([every[::16], edge])
    pick = rng.permutation(np.concatenate([pick, pick[:40], edge]))  # duplicates tie on key and start
    full, every_dev = make_engine(sba, K)
    np.testing.assert_array_equal(every_dev, every)
    e, st = make_engine(sba, K, K, starts=pick)
    n = len(st)
    assert n == len(pick) and n * 8 < sba_len, "per-k-mer path"
    assert {0, 31, 32, 63} <= set((st % 64).tolist()) and st.max() == every[-1] and len(np.unique(st)) < n
    raised = set()
    for label, filt in groupref.filter_cases(K):
        want = check(e, sba, st, K, filt, **HIST)
        check(e, sba, st, K, filt, **PAIRS)
        check(e, sba, st, K, filt)
        if want[0] == "raise":
            raised.add(filt[0])
            continue
        if groupref.filter_eval(sba, every, *filt)[1].any():
            continue  # raises on the whole enumeration: nothing to compare on that path
        res = device_query(full, 0, K, filt, {})
        assert res[0] == "ok"
        passing = every[res[1][0].astype(np.int64)]  # per-position path: the starts that pass
        sub = device_query(e, 0, K, filt, {})
        np.testing.assert_array_equal(st[sub[1][0].astype(np.int64)], st[np.isin(st, passing)], err_msg=label)
    assert raised == {groupref.HOMOPOLYMER, groupref.GC, groupref.NO_AMBIGUOUS}
    # crispr_ngg raises only with starts in the last 22 positions: K = 8 starts
    pick8 = np.concatenate([groupref.enumerate_starts(sba, 8)[::16], [sba_len - 8]]).astype(np.uint32)
    e, st = make_engine(sba, 8, 8, starts=pick8)
    assert len(st) * 8 < sba_len
    want = check(e, sba, st, 8, (groupref.CRISPR_NGG, 0, 0, 0), **HIST)
    assert want[0] == "raise" and want[2] == groupref.FERR_CRISPR_LEN


# ---------------------------------------------------------------------------------------------
# head masks: heads_from_mask_kernel (GK_GROUPS_FROM_HEADS)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2 * TILE + 1903, 3 * TILE + 9])
def test_head_masks(n):
    """Random head masks (density 0.01, 0.5, 1.0) with and without a filter mask (density 0.1,
    0.9): heads set at invalid positions are ignored, a cleared head at the first valid position
    still starts a group."""
    rng = np.random.default_rng(n)
    sba = ACGT[rng.integers(0, 4, n + 7)]
    e, st = make_engine(sba, 8)
    assert len(st) == n and n % 16 != 0
    for density in (0.01, 0.5, 1.0):
        for mask_density in (None, 0.1, 0.9):
            heads = (rng.random(n) < density).astype(np.uint8)
            mask, filt = None, KEEP
            first_valid = 0
            if mask_density is not None:
                mask = (rng.random(n) < mask_density).astype(np.uint8)
                mask[0] = 0
                filt = MASK
                first_valid = int(np.flatnonzero(mask)[0])
                heads[mask == 0] = 1  # heads at invalid positions
                assert heads[:first_valid].all() and first_valid > 0
                e.set_filter_mask(mask)
            heads[first_valid] = 0
            e.set_group_heads(heads)
            want = check(e, sba, st, None, filt, mask=mask, heads=heads, max_counts_bin=300)
            cnt = n if mask is None else int(mask.sum())
            assert want[1][1] == cnt
            if density < 1.0:
                assert want[1][0][2:].sum() > 0 and want[1][0].sum() < cnt
            else:  # every valid k-mer its own group: the cleared head is the first valid k-mer's
                assert want[1][0][1] == cnt
            check(e, sba, st, None, filt, mask=mask, heads=heads, min_group_size=2, yield_first_n=2)
            check(e, sba, st, None, filt, mask=mask, heads=heads)
    e.set_group_heads(np.ones(n + 1, dtype=np.uint8))
    with pytest.raises(_native.GkError) as err:
        e.group_hist(_native.GROUPS_FROM_HEADS, None, _native.GkFilter(0, 0, 0, 0, 0), 1, None, 10)
    assert err.value.code == _native.GK_E_ARG and "head mask length" in err.value.msg
    e.set_group_heads(np.ones(n, dtype=np.uint8))
    e.set_filter_mask(np.ones(n - 1, dtype=np.uint8))
    with pytest.raises(_native.GkError) as err:
        e.group_members(_native.GROUPS_FROM_HEADS, None, _native.GkFilter(*((_native.FILTER_MASK,) + (0,) * 4)), 1,
                        None, None)
    assert err.value.code == _native.GK_E_ARG and "filter mask length" in err.value.msg


# ---------------------------------------------------------------------------------------------
# the chunked tile-sum scan and every grid-stride loop past its grid cap: 4.3 M bases
# ---------------------------------------------------------------------------------------------
LARGE_BASES = 4_300_000


@pytest.fixture(scope="module")
def large():
    """One 4,300,000-base A/C/G/T contig with a 60 k segment copied twice (groups at k = 31),
    sorted at 31: more than 1025 scan tiles, 2,097,152 k-mers and 4,194,304 positions."""
    rng = np.random.default_rng(43)
    sba = ACGT[rng.integers(0, 4, LARGE_BASES)].copy()
    sba[1_000_000:1_060_000] = sba[:60_000]
    sba[3_000_000:3_060_000] = sba[:60_000]
    e, st = make_engine(sba, 31, 31)
    n = len(st)
    assert n == LARGE_BASES - 30 and n > 1025 * TILE and n > 8192 * 256 and LARGE_BASES > 16384 * 256
    return sba, e, st


@pytest.fixture
def chunked_scan(monkeypatch):
    monkeypatch.setitem(_native.options, "GKM_TEST_SCAN_CHUNK", "1024")


def test_large_prefix_histogram(large, chunked_scan):
    """keep-all histogram at kmer_len 12 (masked keys): more than 1,048,576 groups, the histogram
    kernel's grid cap, selected through the chunked tile-sum scan"""
    sba, e, st = large
    want = check(e, sba, st, 12, max_counts_bin=64)
    assert want[1][0].sum() > 4096 * 256 and want[1][0][2:].sum() > 100_000 and want[1][1] == len(st)


def test_large_filtered_yields(large, chunked_scan):
    """GC-filtered first members of the groups of two or more at the sort length: filter_pos_kernel
    past 16,384 blocks of positions, the flag, head and yield kernels past 8,192 blocks, select_flags
    (compaction and group starts) and the yield scan through the chunked tile-sum scan"""
    sba, e, st = large
    passes = fails_some(sba, st, GC31)
    hist, _ = groupref.group_scan(sba, st, 31, valid=passes, max_counts_bin=4)
    assert len(st) > 1025 * TILE and passes.sum() > 8192 * 256 and hist.sum() > 8192 * 256
    want = check(e, sba, st, 31, GC31, min_group_size=2, yield_first_n=1)
    assert len(want[1][0]) > 40_000


def test_large_unsorted_length_filter(large, chunked_scan):
    """Unsorted, length-filtered yields: one group per passing k-mer, 4.3 M yields written through
    the chunked exclusive scan"""
    sba, e, st = large
    filt = (groupref.LENGTH, 40, 0, 0)
    passes = fails_some(sba, st, filt)
    assert len(st) - passes.sum() == 9
    want = check(e, sba, st, 31, filt, is_sorted=False)
    assert len(want[1][0]) == len(st) - 9 > 1025 * TILE


# ---------------------------------------------------------------------------------------------
# gk_locate
# ---------------------------------------------------------------------------------------------
def _contigs(lengths, seed):
    rng = np.random.default_rng(seed)
    seqs = [ACGT[rng.integers(0, 4, L)].tobytes().decode() for L in lengths]
    return seqs, np.frombuffer("$".join(seqs).encode(), dtype=np.uint8)


def _locate_lengths(n_contigs):
    if n_contigs <= 2:
        return [300, 41][:n_contigs]
    lengths = np.random.default_rng(3000).integers(1, 201, n_contigs)
    lengths[[0, 7, 1500, n_contigs - 1]] = 8  # exactly one 8-mer, the first and the last contig among them
    lengths[[1, 2, 3, n_contigs - 2]] = [1, 7, 3, 5]  # no 8-mer
    return lengths.tolist()


@pytest.mark.parametrize("n_contigs", [1, 2, 3000])
def test_locate(n_contigs):
    """locate_kernel's binary search over up to 3,000 segment starts, many segments without a k-mer
    and some with exactly one: start and segment of selected k-mers of the sorted order."""
    lengths = _locate_lengths(n_contigs)
    _, sba = _contigs(lengths, n_contigs)
    seg_starts = groupref.segments_of(sba)
    assert len(seg_starts) == n_contigs
    e, st = make_engine(sba, 8, 8, starts=groupref.enumerate_starts(sba, 8))
    n = len(st)
    seg_of = np.searchsorted(seg_starts, st, "right") - 1
    per_seg = np.bincount(seg_of, minlength=n_contigs)
    if n_contigs == 3000:
        assert (per_seg == 0).sum() > 50 and (per_seg == 1).sum() >= 4 and per_seg[0] == per_seg[-1] == 1
    # sorted positions of the first and the last k-mer of every contig that has one
    pos_of_start = np.empty(len(sba), dtype=np.int64)
    pos_of_start[st] = np.arange(n)
    held = np.flatnonzero(per_seg)
    firsts = pos_of_start[seg_starts[held]]
    lasts = pos_of_start[seg_starts[held] + per_seg[held] - 1]
    rng = np.random.default_rng(n)
    for m in (1, 255, 256, 257, 10_000):
        nums = rng.integers(0, n, m)
        edge = np.concatenate([[0, n - 1, n - 1, 0], firsts[:40], lasts[:40], firsts[-40:], lasts[-40:]])[:m]
        nums[:len(edge)] = edge
        if m == 1:
            nums[0] = n - 1
        sba_idx, seg = e.locate(nums.astype(np.uint64))
        np.testing.assert_array_equal(sba_idx, st[nums])
        np.testing.assert_array_equal(seg, np.searchsorted(seg_starts, st[nums], "right") - 1)
        assert m < 256 or len(np.unique(nums)) < m
    with pytest.raises(_native.GkError) as err:
        e.locate(np.array([0, n], dtype=np.uint64))
    assert err.value.code == _native.GK_E_ARG


@pytest.mark.parametrize("one_based", [False, True])
def test_full_info_over_3000_contigs(one_based):
    """Kmers.get_kmers(kmer_info_to_yield="full") on the 3,000-contig case: record name and position
    of the first member of every group against searchsorted over the segment starts."""
    seqs, sba = _contigs(_locate_lengths(3000), 3000)
    names = [f"rec{i}" for i in range(len(seqs))]
    sc = SequenceCollection(sequence_list=list(zip(names, seqs)))
    np.testing.assert_array_equal(sc.forward_sba, sba)
    seg_starts = groupref.segments_of(sba).astype(np.int64)
    km = gk.Kmers(sc, min_kmer_len=1, max_kmer_len=8)
    km.kmer_sba_start_indices = groupref.enumerate_starts(sba, 8)
    km.sort()
    st = km.kmer_sba_start_indices
    num, y, t = groupref.group_scan(sba, st, 8, yield_first_n=1)
    assert len(num) > TILE
    got = list(km.get_kmers(8, one_based_seq_index=one_based, kmer_info_to_yield="full", yield_first_n=1))
    start = st[num.astype(np.int64)].astype(np.int64)
    seg = np.searchsorted(seg_starts, start, "right") - 1
    assert len(np.unique(seg)) > 2000
    want = [(int(a), "+", names[s], int(p), 8, int(b), int(c))
            for a, s, p, b, c in zip(num, seg, start - seg_starts[seg] + int(one_based), y, t)]
    assert got == want
