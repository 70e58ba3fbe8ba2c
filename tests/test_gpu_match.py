"""Matching statistics on the device: gk_match through Kmers.match_lengths, Kmers.maximal_matches and
_native.Engine.match, on both paths (bytes, keys).

Every expectation comes from tests/matchref.py (numpy on the host sba: the indexed k-mers as rows of
bytes, sets of their prefixes per length, bisection on the sorted rows; pinned to a pure-Python brute
force by tests/test_matchref.py) and never from the code under test.  Every parametrised case first
asserts on that reference alone that it is not trivial.  T mirrors the kernel's tile (gkm_match.hip:
kMatchThreads threads of GKM_MATCH_WIN positions each), BOUNDS the sequence ends one pass keeps in LDS
(kMatchBounds); tests/test_match_host.py checks both against the source.
"""

import ctypes
import re
from functools import lru_cache

import numpy as np
import pytest

import matchref
from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.kmers import MatchResult, maximal_from_lengths  # noqa: F401  (the feature under test)
from genome_kmers.sequence_collection import SequenceCollection

pytestmark = pytest.mark.gpu

WIN = 4          # GKM_MATCH_WIN: positions per thread
T = 256 * WIN    # kMatchTile: positions per block
BOUNDS = 256     # kMatchBounds
CASES = {c["name"]: c for c in load_manifest()}
PER_POS = ("lengths", "first", "count")
PER_READ = ("longest", "longest_pos", "sum_len")
DTYPES = {"lengths": np.uint32, "first": np.uint64, "count": np.uint32, "longest": np.uint32,
          "longest_pos": np.uint32, "sum_len": np.uint64, "offsets": np.uint64}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# genomes (2e4 to 2e5 bases), built once
# ---------------------------------------------------------------------------------------------
def rand_seq(seed, n, letters="ACGT") -> str:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters.encode(), dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


def mutate(seq: str, seed, every=40) -> str:
    """A substitution about every ``every`` bases (A->C->G->T->A)."""
    rng = np.random.default_rng(seed)
    s = bytearray(seq.encode())
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    for p in np.flatnonzero(rng.integers(0, every, len(s)) == 0).tolist():
        s[p] = nxt.get(s[p], 65)
    return s.decode()


@lru_cache(maxsize=None)
def genome(name):
    """[(contig name, str)].  "acgt": 3e4 random bases with a poly-A region (a range far larger than a
    tile), a segment that occurs twice and an all-T contig (the all-T 32-mer: key 2^64 - 1).  "cut": the
    same with contigs of 5, 9 and 20 bases (for sorts with min_kmer_len below them).  "acg": no T but
    one all-T contig of 32 bases: in no k-mer does a T follow another letter.  "cg": C and G only, so
    that reads of A sort below every k-mer and reads of T above.  "one": one contig of 12 bases.  "mixed": the golden IUPAC genome (N
    runs, IUPAC letters) beside random contigs.  "big": 2e5."""
    if name in ("acgt", "acg", "cut"):
        letters = "ACG" if name == "acg" else "ACGT"
        a, b, c = rand_seq(11, 12000, letters), rand_seq(12, 9000, letters), rand_seq(13, 8000, letters)
        main = a + "A" * 3000 + b + a[3000:3700] + c + rand_seq(14, 500, letters)
        short = [("s5", a[40:45]), ("s9", a[60:69]), ("s20", a[80:100])] if name == "cut" else []
        return [("main", main), ("polyT", "T" * (32 if name == "acg" else 70)), ("tail", rand_seq(15, 900, letters))] + short
    if name == "cg":
        return [("main", rand_seq(16, 20000, "CG")), ("tail", rand_seq(17, 300, "CG"))]
    if name == "one":
        return [("only", "CGTACGGATCGA")]
    if name == "mixed":
        gold = seq_list_of(CASES["iupac_k31"], load_case("iupac_k31"))
        r = rand_seq(21, 9000)
        return gold + [("r0", r), ("r1", r[2000:2600] + "NNNNNNNNNNNNNNNN" + rand_seq(22, 3000) + "RYKM" + r[100:400]),
                       ("gold_again", gold[0][1])]
    if name == "big":
        a = rand_seq(31, 150000)
        return [("c0", a), ("c1", a[5000:9000] + rand_seq(32, 46000))]
    raise KeyError(name)


def sba_of(name):
    return matchref.as_sba(genome(name))


def is_acgt(name) -> bool:
    return all(set(s) <= set("ACGT") for _, s in genome(name))


@lru_cache(maxsize=None)
def index_of(name, min_len, max_len, cap):
    return matchref.Index(sba_of(name), min_len, max_len, cap)


@lru_cache(maxsize=None)
def sorted_kmers(name, K, min_len=None, order="stable"):
    """K None: the suffix order (min_len required)."""
    sc = SequenceCollection(sequence_list=genome(name), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K if min_len is None else min_len, max_kmer_len=K)
    km.sort(order=order)
    return km


def keys_eligible(name, K, min_len=None) -> bool:
    """The key path serves the index: ACGT-only, one length of at most 32 bases, a forward sort."""
    return is_acgt(name) and K is not None and K <= 32 and min_len in (None, K)


def force(monkeypatch, path):
    if path == "auto":
        monkeypatch.delitem(_native.options, "GKM_MATCH_PATH", raising=False)
    else:
        monkeypatch.setitem(_native.options, "GKM_MATCH_PATH", path)


def expect(name, K, reads, min_len=None, cap=None):
    cap = K if cap is None else cap
    return matchref.match(index_of(name, K if min_len is None else min_len, K, cap), reads)


def assert_equal(res, ref, note="", outs=PER_POS + PER_READ + ("offsets",)):
    for out in outs:
        got = getattr(res, out)
        assert got.dtype == DTYPES[out], f"{note} {out}"
        np.testing.assert_array_equal(got, ref[out], err_msg=f"{note} {out}")


def check(monkeypatch, name, K, reads, min_len=None, cap=None, order="stable", paths=None, ref=None, totals=True):
    """Kmers.match_lengths on each path (forced, and the call's own choice) equals the reference on
    all outputs; the totals-only call returns the same per-read arrays."""
    if ref is None:
        ref = expect(name, K, reads, min_len, cap)
    km = sorted_kmers(name, K, min_len, order)
    if paths is None:
        paths = ("auto", "bytes", "keys") if keys_eligible(name, K, min_len) and order == "stable" else ("auto", "bytes")
    for path in paths:
        force(monkeypatch, path)
        assert_equal(km.match_lengths(reads, max_len=cap), ref, f"{name} K={K} cap={cap} {path}")
    if totals:
        force(monkeypatch, "auto")
        res = km.match_lengths(reads, max_len=cap, per_position=False)
        assert res.lengths is None and res.first is None and res.count is None and res.offsets is None
        assert_equal(res, ref, "totals only", PER_READ)
    return ref, km


def sample_reads(name, seed, n, length, n_every=0):
    """n reads: two thirds cut from the genome with substitutions, a third random; every
    ``n_every``-th read gets one N."""
    rng = np.random.default_rng(seed)
    contigs = [s for _, s in genome(name) if len(s) > length]
    reads = []
    for i in range(n):
        src = contigs[int(rng.integers(0, len(contigs)))]
        at = int(rng.integers(0, len(src) - length))
        r = mutate(src[at:at + length], seed * 1000 + i) if i % 3 else rand_seq(seed * 1000 + i, length)
        if n_every and i % n_every == 0:
            p = int(rng.integers(0, length))
            r = r[:p] + "N" + r[p + 1:]
        reads.append(r)
    return reads


def nontrivial(ref, cap, zeros=True) -> bool:
    """Matches at the cap, positions without a match (``zeros``: on a genome that holds every letter of
    the reads there are none), lengths strictly between, a count above 1."""
    v = ref["lengths"]
    return bool((v == cap).any() and ((v == 0).any() or not zeros) and ((v > 0) & (v < cap)).any()
                and (ref["count"] > 1).any())


# ---------------------------------------------------------------------------------------------
# 1. every value of the length
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dir_on", [True, False])
@pytest.mark.parametrize("K", [3, 12, 31, 32])
def test_every_length(K, dir_on, monkeypatch):
    """Reads g[i:i + l] + "T" against a genome in which no T follows another letter: the first position
    of read l matches exactly l bases, for every l in 0..K (around D / 2 = 11 symbols, where the prefix's range
    comes from the directory alone or from a search; K = 3, where D = 2 K); GKM_LOOKUP_DIR=0 searches
    without the directory."""
    main = genome("acg")[0][1]
    rng = np.random.default_rng(K)
    reads = []
    for l in range(K + 1):
        for i in rng.integers(0, 20000, 3).tolist():
            reads.append(main[i:i + l] + "T")
    reads.append("NAN")
    ref = expect("acg", K, reads)
    firsts = ref["lengths"][ref["offsets"][:-2].astype(np.int64)]
    assert firsts.tolist() == [max(l, 1) for l in range(K + 1) for _ in range(3)]  # (a lone "T" matches the all-T contig)  # every value occurs, on the reference alone
    assert sorted(set(ref["lengths"].tolist())) == list(range(K + 1)) and (ref["count"] > 1).any()
    if not dir_on:
        monkeypatch.setitem(_native.options, "GKM_LOOKUP_DIR", "0")
    check(monkeypatch, "acg", K, reads, ref=ref, totals=dir_on)


@pytest.mark.parametrize("K,cap", [(31, 12), (31, 1), (12, 11), (32, 31)])
def test_max_len_below_k(K, cap, monkeypatch):
    reads = sample_reads("acgt", 3, 40, 100, n_every=4) + ["A" * 50, "T" * 40, "ACG"]
    ref = expect("acgt", K, reads, cap=cap)
    v = ref["lengths"]
    assert (v == cap).any() and (ref["count"] > 1).any() and ((v < cap).any())
    check(monkeypatch, "acgt", K, reads, cap=cap, ref=ref)


# ---------------------------------------------------------------------------------------------
# 2. neighbours of the insertion point
# ---------------------------------------------------------------------------------------------
def test_below_and_above_every_key(monkeypatch):
    K = 12
    main = genome("cg")[0][1]
    reads = ["A" * 30, "T" * 30, main[100:130], "CCGA" + "T" * 10, mutate(main[500:600], 5), "GGGGGGGGGGGGGGGGT", "CA", "GT"]
    ref = expect("cg", K, reads)
    index = index_of("cg", K, K, K)
    off = ref["offsets"].astype(np.int64)
    assert not ref["lengths"][off[0]:off[1]].any() and not ref["lengths"][off[1]:off[2]].any()
    assert index.sorted[0] > b"A" * K and index.sorted[-1] < b"T" * K  # below the first key, above the last
    assert nontrivial(ref, K)
    check(monkeypatch, "cg", K, reads, ref=ref)


def test_index_of_one_kmer(monkeypatch):
    K = 12
    only = genome("one")[0][1]
    reads = [only, only[:7] + "T" + only[8:], "A" * 14, "T" * 14, only[3:], "CGTACGGATCGAC", "", "CGTT", "D"]
    ref = expect("one", K, reads)
    assert index_of("one", K, K, K).n == 1 and ref["longest"].tolist()[:2] == [12, 7] and ref["count"].max() == 1
    check(monkeypatch, "one", K, reads, ref=ref, paths=("auto", "bytes"))  # (a sort of one k-mer leaves no final keys)


@pytest.mark.parametrize("K", [12, 31])
def test_predecessor_successor_and_both(K, monkeypatch):
    reads = sample_reads("acgt", 17, 30, 90, n_every=5)
    ref = expect("acgt", K, reads)
    sides = matchref.neighbour_sides(index_of("acgt", K, K, K), reads)
    for side in (matchref.PREV, matchref.NEXT, matchref.PREV | matchref.NEXT):
        assert (sides == side).any()  # the predecessor alone, the successor alone, both attain the maximum
    assert nontrivial(ref, K)
    check(monkeypatch, "acgt", K, reads, ref=ref)


def test_all_a_and_all_t_32mers_and_the_poly_a_range(monkeypatch):
    """Keys 0 and 2^64 - 1 at K = 32; inside the poly-A region the range of a match is far larger than
    a tile."""
    K = 32
    main = genome("acgt")[0][1]
    reads = ["A" * 100, "T" * 69, "T" * 32 + "A" * 32 + "C", "A" * 31 + "C" + "T" * 40, main[11990:12040], main[14980:15030],
             "G" + "T" * 31, "C" + "A" * 40, "NAN"]
    ref = expect("acgt", K, reads)
    index = index_of("acgt", K, K, K)
    assert index.sorted[0] == b"A" * K and index.sorted[-1] == b"T" * K
    assert ref["count"].max() > 2 * T and nontrivial(ref, K)
    check(monkeypatch, "acgt", K, reads, ref=ref)


def test_genome_of_2e5_bases(monkeypatch):
    K = 31
    reads = sample_reads("big", 23, 60, 150, n_every=7)
    ref = expect("big", K, reads)
    assert nontrivial(ref, K)
    check(monkeypatch, "big", K, reads, ref=ref)


# ---------------------------------------------------------------------------------------------
# 3. read geometry: tiles, the LDS table, chunks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [12, 31])
def test_tile_edge_sweep(K, monkeypatch):
    """A read boundary, an N and the batch's end swept across the tile edge, a whole match length
    either side of it."""
    main = genome("acgt")[0][1]
    for d in (-K - 1, -K, -K + 1, -2, -1, 0, 1, 2):
        first = main[200:200 + T + d]
        with_n = main[5000:5000 + T + d] + "N" + main[6000:6040]
        for reads in ([first, main[3000:3080]], [with_n], [main[7000:7000 + T + d]], [first[:-1], "", "", main[3000:3050]]):
            ref = expect("acgt", K, reads)
            assert (ref["lengths"] == K).any() and (ref["lengths"] < K).any()
            check(monkeypatch, "acgt", K, reads, ref=ref, paths=("keys", "bytes"), totals=False)


def test_read_across_more_than_three_tiles(monkeypatch):
    K = 31
    main = genome("acgt")[0][1]
    long_read = "GN" + mutate(main[1000:1000 + 3 * T + 500], 3, every=60)
    reads = [main[50:90], long_read, "ACGN", "", mutate(main[20000:20000 + T + 7], 4)]
    ref = expect("acgt", K, reads)
    assert nontrivial(ref, K) and ref["longest_pos"][1] > 0
    check(monkeypatch, "acgt", K, reads, ref=ref)


@pytest.mark.parametrize("K", [3, 12])
def test_more_boundaries_than_the_lds_table(K, monkeypatch):
    """Tiles with more read ends than one pass keeps: reads of 0 to 3 bases, and reads shorter than the
    cap throughout."""
    main = genome("acgt")[0][1]
    rng = np.random.default_rng(K)
    reads = [main[100:160]]
    for i in range(3 * BOUNDS + 50):
        at = int(rng.integers(0, 20000))
        reads.append(main[at:at + int(rng.integers(0, 4))] if i % 7 else "N")
    reads += [main[400:1700], ""] + [main[at:at + 2] for at in range(0, 2 * BOUNDS * 3, 3)] + [main[900:960]]
    ref = expect("acgt", K, reads)
    ends = ref["offsets"][1:].astype(np.int64)
    assert np.bincount(ends // T).max() > 2 * BOUNDS  # on the reference's offsets alone
    assert (ref["lengths"] == K).any() and (ref["lengths"] == 0).any() and (ref["longest"] < K).any()
    check(monkeypatch, "acgt", K, reads, ref=ref)


@pytest.mark.parametrize("K,cap", [(12, None), (31, None), (31, 9)])
def test_chunk_edge_sweep(K, cap, monkeypatch):
    """Chunk ends swept through the C - 1 overlap: every chunk size from one match up, then sizes
    around a tile; the answers equal the single-chunk ones."""
    C = K if cap is None else cap
    main = genome("acgt")[0][1]
    reads = [main[100:250], "", mutate(main[2000:2300], 8), main[12100:12100 + 2 * C], "ACGTN" * 7, main[300:300 + C - 1],
             mutate(main[9000:9400], 9)]
    ref = expect("acgt", K, reads, cap=cap)
    assert nontrivial(ref, C)
    for chunk in list(range(C, 2 * C + 2)) + [97, 256, T - 1, T, T + 1, T + C - 1, T + C]:
        monkeypatch.setitem(_native.options, "GKM_MATCH_CHUNK", str(chunk))
        check(monkeypatch, "acgt", K, reads, cap=cap, ref=ref, paths=("keys", "bytes"), totals=chunk % 2 == 0)


def test_many_chunks_of_a_larger_batch(monkeypatch):
    K = 31
    reads = sample_reads("acgt", 29, 120, 150, n_every=9) + ["", "A" * 200]
    ref = expect("acgt", K, reads)
    assert nontrivial(ref, K)
    for chunk in (None, 5000, 1500):
        if chunk:
            monkeypatch.setitem(_native.options, "GKM_MATCH_CHUNK", str(chunk))
        check(monkeypatch, "acgt", K, reads, ref=ref)


# ---------------------------------------------------------------------------------------------
# 4. the byte path alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [12, 31])
def test_mixed_genome(K, monkeypatch):
    """N matches N, IUPAC letters match themselves, and nothing else."""
    r1 = genome("mixed")[-2][1]
    reads = sample_reads("mixed", 31, 40, 120, n_every=3) + [r1[580:640], r1[3610:3640], "N" * 40, "RYKMACGT"]
    ref = expect("mixed", K, reads)
    arr, off = matchref.pack(reads)
    assert nontrivial(ref, K, zeros=False) and (ref["lengths"][arr == ord("N")] > 1).any()
    check(monkeypatch, "mixed", K, reads, ref=ref)
    force(monkeypatch, "keys")
    with pytest.raises(_native.GkError, match="GKM_MATCH_PATH=keys") as e:
        sorted_kmers("mixed", K).match_lengths(reads)
    assert e.value.code == _native.GK_E_UNSUPPORTED


@pytest.mark.parametrize("K", [40, 63])
def test_long_kmers(K, monkeypatch):
    reads = sample_reads("acgt", 37, 30, 200, n_every=6) + ["A" * 100]
    ref = expect("acgt", K, reads)
    assert nontrivial(ref, K)
    check(monkeypatch, "acgt", K, reads, ref=ref)


@pytest.mark.parametrize("name,min_len,K", [("cut", 4, 12), ("cut", 1, 31), ("mixed", 8, 21)])
def test_min_below_max(name, min_len, K, monkeypatch):
    """k-mers cut short by contig ends are in the index: a read that runs past a contig's end matches
    up to it, and the cut k-mers sort below their extensions."""
    tail = genome(name)[0][1][-(K - 2):]
    s9 = genome("cut")[4][1]
    reads = sample_reads(name, 41, 30, 100, n_every=5) + [tail + "ACGTACGT", s9 + "T", s9[2:], tail[3:]]
    ref = expect(name, K, reads, min_len=min_len)
    index = index_of(name, min_len, K, K)
    assert (index.lens < K).any() and nontrivial(ref, K, zeros=name != "mixed")
    no_cut = expect(name, K, reads)  # the same reads against whole k-mers only differ
    assert (no_cut["lengths"] != ref["lengths"]).any()
    check(monkeypatch, name, K, reads, min_len=min_len, ref=ref)


@pytest.mark.parametrize("name,min_len,cap", [("cut", 5, 12), ("cut", 1, 40), ("mixed", 3, 40)])
def test_suffix_order_with_a_cap(name, min_len, cap, monkeypatch):
    reads = sample_reads(name, 43, 30, 120, n_every=5) + ["A" * 100, genome(name)[0][1][-20:] + "ACGT"]
    ref = matchref.match(index_of(name, min_len, None, cap), reads)
    assert nontrivial(ref, cap, zeros=name != "mixed")
    km = sorted_kmers(name, None, min_len)
    for path in ("auto", "bytes"):
        force(monkeypatch, path)
        assert_equal(km.match_lengths(reads, max_len=cap), ref, f"{name} None cap={cap} {path}")
    assert_equal(km.match_lengths(reads, max_len=cap, per_position=False), ref, "totals", PER_READ)


@pytest.mark.parametrize("name,K", [("acgt", 12), ("mixed", 21)])
def test_after_reference_order_sorts(name, K, monkeypatch):
    reads = sample_reads(name, 47, 40, 120, n_every=6) + ["A" * 40]
    ref = expect(name, K, reads)
    assert nontrivial(ref, K, zeros=name != "mixed")
    check(monkeypatch, name, K, reads, order="reference", ref=ref)


# ---------------------------------------------------------------------------------------------
# 5. cross-checks through the library
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,min_len", [("acgt", 31, None), ("cut", 12, 4), ("mixed", 21, None)])
def test_ranges_equal_find(name, K, min_len, monkeypatch):
    reads = sample_reads(name, 53, 30, 110, n_every=4)
    km = sorted_kmers(name, K, min_len)
    res = km.match_lengths(reads)
    arr, off = _native.pack_sequences(reads)
    rng = np.random.default_rng(3)
    raw = arr.tobytes()
    checked_longer = 0
    for p in rng.choice(len(arr), 150, replace=False).tolist():
        j = int(np.searchsorted(off, p, side="right")) - 1
        m = min(K, int(off[j + 1]) - p)
        l = int(res.lengths[p])
        assert 0 <= l <= m
        if l:
            assert km.find(raw[p:p + l]) == (int(res.first[p]), int(res.count[p])) and res.count[p] > 0
        else:
            assert (int(res.first[p]), int(res.count[p])) == (0, 0)
        if l < m and _native._QUERY_OK[arr[p:p + l + 1]].all():
            assert km.find(raw[p:p + l + 1])[1] == 0
            checked_longer += 1
    assert checked_longer > 10
    # the per-read outputs are reductions of the per-position arrays
    for j in range(len(reads)):
        v = res.lengths[int(off[j]):int(off[j + 1])].astype(np.int64)
        assert res.longest[j] == v.max() and res.sum_len[j] == v.sum() and res.longest_pos[j] == int(np.argmax(v))


@pytest.mark.parametrize("name,K", [("acgt", 31), ("mixed", 21)])
def test_counts_at_full_length_equal_the_screen(name, K, monkeypatch):
    reads = sample_reads(name, 59, 40, 130, n_every=0)
    km = sorted_kmers(name, K)
    res = km.match_lengths(reads)
    wc = km.screen(reads, per_window=True).window_counts
    full = res.lengths == K
    assert full.any() and (~full).any()
    np.testing.assert_array_equal(res.count[full], wc[full])
    assert not wc[~full].any()


def test_maximal_matches(monkeypatch):
    K = 31
    reads = sample_reads("acgt", 61, 30, 150, n_every=0)
    ref = expect("acgt", K, reads)
    km = sorted_kmers("acgt", K)
    read, pos, length, first, count = km.maximal_matches(reads, 20)
    want = matchref.maximal(ref["lengths"], ref["offsets"], 20)
    assert len(want[0]) > 10
    for got, w in zip((read, pos, length), want):
        np.testing.assert_array_equal(got, w)
    at = ref["offsets"].astype(np.int64)[read] + pos
    np.testing.assert_array_equal(first, ref["first"][at])
    np.testing.assert_array_equal(count, ref["count"][at])
    # the seeds' locations, through the existing locate: the genome holds the match there
    sba = sba_of("acgt").tobytes()
    arr = matchref.pack(reads)[0].tobytes()
    for i in range(0, len(read), 7):
        starts = km.kmer_sba_start_indices[int(first[i]):int(first[i] + count[i])]
        for s in starts.tolist():
            assert sba[s:s + int(length[i])] == arr[int(at[i]):int(at[i]) + int(length[i])]


# ---------------------------------------------------------------------------------------------
# 6. the interface
# ---------------------------------------------------------------------------------------------
def fresh_kmers(K, max_len="K", sort=False, canonical=False):
    sc = SequenceCollection(sequence_list=[("c", rand_seq(1, 500))], strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K, max_kmer_len=K if max_len == "K" else max_len)
    if sort:
        km.sort(canonical=canonical)
    return km


def raw_match(km, arr, off, max_len=0, flags=0, null_seqs=False, null_out=False):
    """gk_match through the C binding with the arrays as given (no pack_sequences, no host checks)."""
    km._sync_device()
    eng = km._get_engine()
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    nseq = off.size - 1
    longest = np.full(max(nseq, 1), 77, dtype=np.uint32)
    pos = np.full(max(nseq, 1), 77, dtype=np.uint32)
    total = np.full(max(nseq, 1), 77, dtype=np.uint64)
    rc = eng.lib.gk_match(eng.ctx, None if null_seqs else _native._ptr(arr, ctypes.c_uint8),
                          _native._ptr(off, ctypes.c_uint64), nseq, max_len, flags,
                          None if null_out else _native._ptr(longest, ctypes.c_uint32), _native._ptr(pos, ctypes.c_uint32),
                          _native._ptr(total, ctypes.c_uint64), None, None, None)
    msg = eng.lib.gk_last_error(eng.ctx)
    return rc, (msg.decode() if msg else ""), longest, pos, total


def test_each_per_position_array_may_be_null(monkeypatch):
    K = 31
    reads = sample_reads("acgt", 67, 30, 140, n_every=5)
    ref = expect("acgt", K, reads)
    km = sorted_kmers("acgt", K)
    arr, off = _native.pack_sequences(reads)
    names = ("longest", "longest_pos", "sum_len") + PER_POS
    for path in ("keys", "bytes"):
        force(monkeypatch, path)
        for chunk in (None, 700):
            if chunk:
                monkeypatch.setitem(_native.options, "GKM_MATCH_CHUNK", str(chunk))
            for want in ((False, True, True), (True, False, True), (True, True, False), (True, False, False),
                         (False, False, True)):
                got = km._engine.match(arr, off, 0, want)
                for name, value in zip(names, got):
                    if name in PER_POS and not want[PER_POS.index(name)]:
                        assert value is None
                    else:
                        np.testing.assert_array_equal(value, ref[name], err_msg=f"{path} {want} {name}")


def test_preconditions():
    reads = ["ACGTACGTACGT"]
    arr, off = _native.pack_sequences(reads)
    km = fresh_kmers(5)
    with pytest.raises(AssertionError, match="must be sorted when calling match_lengths"):
        km.match_lengths(reads)
    rc, msg, *_ = raw_match(km, arr, off)
    assert rc == _native.GK_E_STATE and "not sorted" in msg
    canon = fresh_kmers(5, sort=True, canonical=True)
    with pytest.raises(ValueError, match="needs a forward order: canonical k-mers have no prefixes"):
        canon.match_lengths(reads)
    rc, msg, *_ = raw_match(canon, arr, off)
    assert rc == _native.GK_E_UNSUPPORTED and "canonical k-mers have no prefixes: gk_match needs a forward order" in msg
    km = fresh_kmers(5, sort=True)
    with pytest.raises(ValueError, match=r"max_len \(6\) is greater than max_kmer_len \(5\)"):
        km.match_lengths(reads, max_len=6)
    rc, msg, *_ = raw_match(km, arr, off, max_len=6)
    assert rc == _native.GK_E_ARG and "max_len (6) is above the sort length (5)" in msg
    none = fresh_kmers(2, max_len=None, sort=True)
    with pytest.raises(ValueError, match="needs max_len when max_kmer_len is None"):
        none.match_lengths(reads)
    with pytest.raises(ValueError, match=r"max_len \(4097\) is greater than 4096"):
        none.match_lengths(reads, max_len=4097)
    for bad in (0, 4097):
        rc, msg, *_ = raw_match(none, arr, off, max_len=bad)
        assert rc == _native.GK_E_ARG and f"max_len ({bad}) must be in 1..4096" in msg
    rc, _, longest, _, _ = raw_match(none, arr, off, max_len=4096)
    assert rc == _native.GK_OK and longest[0] <= 12
    for bad_off, what in (([1, 12], "offsets\\[0\\] must be 0"), ([0, 8, 4, 12], "offsets decrease at sequence 1")):
        with pytest.raises(_native.GkError, match=what) as e:
            km._engine.match(arr, np.array(bad_off, dtype=np.uint64))
        assert e.value.code == _native.GK_E_ARG
    with pytest.raises(ValueError, match="offsets must"):
        km.match_lengths((arr, np.array([0, 8, 4, 12], dtype=np.uint64)))
    # an over-long sequence: refused from the offsets alone, before any byte is read (there are none)
    rc, msg, *_ = raw_match(km, arr, [0, 1 << 32], null_seqs=True)
    assert rc == _native.GK_E_ARG and "sequence 0 is longer than 2^32 - 1 bytes" in msg
    rc, msg, *_ = raw_match(km, arr, off, flags=1)
    assert rc == _native.GK_E_ARG and "flags (1) must be 0" in msg
    rc, msg, *_ = raw_match(km, arr, off, null_seqs=True)
    assert rc == _native.GK_E_ARG and "null" in msg
    rc, msg, *_ = raw_match(km, arr, off, null_out=True)
    assert rc == _native.GK_E_ARG and "null" in msg
    # nseq == 0 touches nothing, a context in any state included
    rc, _, longest, pos, total = raw_match(fresh_kmers(5), arr, [0])
    assert rc == _native.GK_OK and longest[0] == 77 and pos[0] == 77 and total[0] == 77
    # a total length of 0 writes zeros over whatever the arrays held
    rc, _, longest, pos, total = raw_match(km, np.zeros(0, dtype=np.uint8), [0, 0, 0])
    assert rc == _native.GK_OK and not longest.any() and not pos.any() and not total.any()


def test_path_knob_values(monkeypatch):
    km = sorted_kmers("acgt", 12)
    monkeypatch.setitem(_native.options, "GKM_MATCH_PATH", "key")
    with pytest.raises(_native.GkError, match="GKM_MATCH_PATH must be 'bytes' or 'keys'") as e:
        km.match_lengths("ACGTACGTACGTACGT")
    assert e.value.code == _native.GK_E_ARG
    monkeypatch.setitem(_native.options, "GKM_MATCH_PATH", "keys")
    with pytest.raises(_native.GkError, match="GKM_MATCH_PATH=keys") as e:
        sorted_kmers("acgt", 40).match_lengths("ACGTACGTACGTACGT")
    assert e.value.code == _native.GK_E_UNSUPPORTED


@pytest.mark.parametrize("path", ["bytes", "keys"])
def test_bytes_outside_the_alphabet(path, monkeypatch):
    """Lower case and '$', found on the device: gk_screen's message, also when the byte lies in a
    later chunk."""
    K = 12
    km = sorted_kmers("acgt", K)
    main = genome("acgt")[0][1]
    reads = [main[100:400], "", main[500:800], main[900:1500]]
    arr, off = _native.pack_sequences(reads)
    force(monkeypatch, path)
    for chunk in (None, 256):
        if chunk:
            monkeypatch.setitem(_native.options, "GKM_MATCH_CHUNK", str(chunk))
        for seq, at, byte in ((0, 0, "a"), (2, 17, "$"), (3, 599, "c"), (2, 299, "n")):
            bad = arr.copy()
            bad[int(off[seq]) + at] = ord(byte)
            want = re.escape(f"sequence {seq} holds byte 0x{ord(byte):02x} ('{byte}') at offset {at},")
            with pytest.raises(_native.GkError, match=want) as e:
                km._engine.match(bad, off)
            assert e.value.code == _native.GK_E_ALPHABET
        two = arr.copy()  # the first bad byte is the one named
        two[int(off[3]) + 5] = ord("x")
        two[int(off[2]) + 250] = ord("y")
        with pytest.raises(_native.GkError, match="sequence 2 holds byte 0x79 .* at offset 250,"):
            km._engine.match(two, off)
        # the context serves the next call
        assert_equal(km.match_lengths(reads), expect("acgt", K, reads), "after an error")


def test_empty_batches_and_input_forms(monkeypatch):
    km = sorted_kmers("acgt", 12)
    main = genome("acgt")[0][1]
    for path in ("auto", "bytes", "keys"):
        force(monkeypatch, path)
        res = km.match_lengths([])
        assert all(len(getattr(res, out)) == 0 for out in PER_POS + PER_READ) and res.offsets.tolist() == [0]
        res = km.match_lengths(["", "", ""])
        assert res.longest.tolist() == [0, 0, 0] and res.sum_len.tolist() == [0, 0, 0] and len(res.lengths) == 0
        res = km.match_lengths("")
        assert res.longest.tolist() == [0] and res.longest_pos.tolist() == [0]
    ref = expect("acgt", 12, [main[100:160]])
    assert_equal(km.match_lengths(main[100:160]), ref)
    assert_equal(km.match_lengths(main[100:160].encode()), ref)
    assert_equal(km.match_lengths(_native.pack_sequences([main[100:160]])), ref)
    assert isinstance(km.match_lengths(main[100:160]), MatchResult)


def test_match_disturbs_nothing(monkeypatch):
    """find, get_unique_kmers, count_in and lcp give the same after a match as before; the join
    result and the LCP view are still on the device."""
    K = 12
    km = sorted_kmers("acgt", K)
    other = sorted_kmers("acg", K)
    main = genome("acgt")[0][1]
    queries = [main[i:i + K] for i in range(0, 3000, 97)] + ["A" * K, "T" * K, "ACGTTGCAACGT"]
    reads = sample_reads("acgt", 9, 50, 150, n_every=5)
    ref = expect("acgt", K, reads)
    before = (km.find(queries), km.get_unique_kmers(), km.count_in(other), km.kmer_sba_start_indices.copy())
    for path in ("keys", "bytes"):
        force(monkeypatch, path)
        lcp_before = km.lcp()
        view_before = km._engine.device_lcp()
        assert_equal(km.match_lengths(reads), ref, path)
        first, count = km._engine.join_result()  # the join result is still there
        np.testing.assert_array_equal(first, before[2][0])
        np.testing.assert_array_equal(count, before[2][1])
        assert km._engine.device_lcp() == view_before  # ... and the LCP view
        out = np.empty(view_before[1], dtype=np.uint32)
        km._engine._check(km._engine.lib.gk_copy_lcp(km._engine.ctx, 0, _native._ptr(out, ctypes.c_uint32), len(out)))
        np.testing.assert_array_equal(out, lcp_before)
        after = (km.find(queries), km.get_unique_kmers(), km.count_in(other), km.kmer_sba_start_indices)
        for b, a in zip(before[:3], after[:3]):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(after[3], before[3])
        assert_equal(km.match_lengths(reads), ref, path + " again")
