"""The read screen on the device: gk_screen through Kmers.screen and _native.Engine.screen, on both
paths (bytes, keys).

Every expectation comes from tests/screenref.py (numpy on the host sba: windows without '$', the
canonical form by a complement table spelt out there, np.unique with counts, then the reads' windows
looked up among them) and never from the code under test.  Every parametrised case first asserts on
that reference alone that it is not trivial: some windows present, some absent, some with a count
above 1.  T mirrors the kernel's tile (gkm_screen.hip: kScreenThreads threads of kScreenWin windows
each), BOUNDS the sequence ends one pass keeps in LDS (kScreenBounds).
"""

import re
from functools import lru_cache

import numpy as np
import pytest

import screenref
from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection

pytestmark = pytest.mark.gpu

WIN = 4          # kScreenWin: windows per thread
T = 256 * WIN    # kScreenTile: positions per block
BOUNDS = 256     # kScreenBounds
CASES = {c["name"]: c for c in load_manifest()}
OUTPUTS = ("n_windows", "n_present", "occurrences", "window_counts", "offsets")


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


PALINDROME = "ACGTACGTACGT"  # its own reverse complement (K = 12)


@lru_cache(maxsize=None)
def genome(name):
    """[(contig name, str)].  "acgt": 3e4 random bases with a poly-A region (its all-A windows have a
    count far above 1), a segment that occurs twice, two copies of PALINDROME and an all-T contig
    (the all-T 32-mer: key 2^64 - 1).  "acg": no T but one all-T contig, so that 3-mers are absent.
    "mixed": the golden IUPAC genome (N runs, IUPAC letters) beside random contigs.  "big": 2e5."""
    if name in ("acgt", "acg"):
        letters = "ACGT" if name == "acgt" else "ACG"
        a, b, c = rand_seq(11, 12000, letters), rand_seq(12, 9000, letters), rand_seq(13, 8000, letters)
        main = a + "A" * 200 + b + PALINDROME + a[3000:3700] + c + PALINDROME + rand_seq(14, 500, letters)
        return [("main", main), ("polyT", "T" * 70), ("tail", rand_seq(15, 900, letters))]
    if name == "mixed":
        gold = seq_list_of(CASES["iupac_k31"], load_case("iupac_k31"))
        r = rand_seq(21, 9000)
        return gold + [("r0", r), ("r1", r[2000:2600] + "NNNNNNNNNNNNNNNN" + rand_seq(22, 3000) + "RYKM" + r[100:400]),
                       ("gold_again", gold[0][1])]
    if name == "big":
        a = rand_seq(31, 150000)
        return [("c0", a), ("c1", a[5000:9000] + rand_seq(32, 46000))]
    raise KeyError(name)


def occurrences_of(name, kmer: str) -> int:
    """Overlapping occurrences of one k-mer in the genome's contigs, by plain string search."""
    return sum(sum(1 for i in range(len(s) - len(kmer) + 1) if s.startswith(kmer, i)) for _, s in genome(name))


def sba_of(name):
    return screenref.as_sba(genome(name))


def is_acgt(name) -> bool:
    return all(set(s) <= set("ACGT") for _, s in genome(name))


@lru_cache(maxsize=None)
def index_of(name, K, canonical=False):
    return screenref.genome_kmers(sba_of(name), K, canonical)


@lru_cache(maxsize=None)
def sorted_kmers(name, K, canonical=False, order="stable", min_len=None):
    sc = SequenceCollection(sequence_list=genome(name), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K if min_len is None else min_len, max_kmer_len=K)
    km.sort(canonical=canonical, order=order)
    return km


def keys_eligible(name, K, canonical=False, min_len=None) -> bool:
    """The key path serves the index: ACGT-only, one length of at most 32 bases, a forward sort."""
    return is_acgt(name) and K <= 32 and not canonical and min_len in (None, K)


def force(monkeypatch, path):
    if path == "auto":
        monkeypatch.delitem(_native.options, "GKM_SCREEN_PATH", raising=False)
    else:
        monkeypatch.setitem(_native.options, "GKM_SCREEN_PATH", path)


def expect(name, K, reads, canonical=False, both=False):
    return screenref.screen(sba_of(name), K, reads, canonical, both, index=index_of(name, K, canonical))


def assert_equal(res, ref, note=""):
    assert res.n_windows.dtype == np.uint32 and res.n_present.dtype == np.uint32, note
    assert res.occurrences.dtype == np.uint64 and res.window_counts.dtype == np.uint32, note
    for out in OUTPUTS:
        np.testing.assert_array_equal(getattr(res, out), ref[out], err_msg=f"{note} {out}")


def check(monkeypatch, name, K, reads, canonical=False, both=False, min_len=None, order="stable", paths=None,
          ref=None):
    """Kmers.screen on each path (forced, and the call's own choice) equals the reference on all
    outputs; the totals-only call returns the same per-read arrays."""
    if ref is None:
        ref = expect(name, K, reads, canonical, both)
    km = sorted_kmers(name, K, canonical, order, min_len)
    eligible = keys_eligible(name, K, canonical, min_len)
    if paths is None:
        paths = ("auto", "bytes", "keys") if eligible else ("auto", "bytes")
    for path in paths:
        force(monkeypatch, path)
        assert_equal(km.screen(reads, both_strands=both, per_window=True), ref, f"{name} K={K} {path}")
    force(monkeypatch, "auto")
    res = km.screen(reads, both_strands=both)
    assert res.window_counts is None and res.offsets is None
    for out in OUTPUTS[:3]:
        np.testing.assert_array_equal(getattr(res, out), ref[out], err_msg=out)
    return ref, km


def sample_reads(name, seed, n, length, n_every=0):
    """n reads: a third cut from the genome with substitutions, a third from its reverse complement, a
    third random; every ``n_every``-th read gets one N."""
    rng = np.random.default_rng(seed)
    contigs = [s for _, s in genome(name) if len(s) > length]
    reads = []
    for i in range(n):
        src = contigs[int(rng.integers(0, len(contigs)))]
        at = int(rng.integers(0, len(src) - length))
        if i % 3 == 0:
            r = mutate(src[at:at + length], seed * 1000 + i)
        elif i % 3 == 1:
            r = screenref.revcomp(src[at:at + length])
        else:
            r = rand_seq(seed * 1000 + i, length)
        if n_every and i % n_every == 0:
            p = int(rng.integers(0, length))
            r = r[:p] + "N" + r[p + 1:]
        reads.append(r)
    return reads


# ---------------------------------------------------------------------------------------------
# 1. both paths, bit-identical with the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [3, 11, 12, 31, 32])
def test_both_paths(K, both, monkeypatch):
    """2K below, at and above the directory's 22 bits (the directory indexes min(22, 2K) bits, so at
    K = 3 a bucket is one 3-mer and the searches inside it end at once); K = 32 (mask 2^64 - 1, the
    all-T key)."""
    name = "acg" if K < 8 else "acgt"
    main = genome(name)[0][1]
    reads = sample_reads(name, 100 + K, 60, 150, n_every=7)
    reads += ["A" * 40, "T" * 40, "A" * 31 + "C", main[11990:12230], "T" * 32 + "G" + "T" * 32, "", main[:K],
              "A" * 250, main[12190:12190 + K + 1], "ACGT" * 20, "N" * 50]
    ref = expect(name, K, reads, both=both)
    assert screenref.nontrivial(ref)
    polya = int(ref["window_counts"][ref["offsets"][60]])  # the all-A window of the read "A" * 40
    assert polya >= 200 - K + 1
    assert int(ref["occurrences"].max()) > 1000  # a read that sums many occurrences
    check(monkeypatch, name, K, reads, both=both, ref=ref)


def test_all_a_and_all_t_32mers(monkeypatch):
    """Keys 0 and 2^64 - 1 at K = 32, found on the key path."""
    reads = ["A" * 32, "T" * 32, "T" * 33, "A" * 31 + "T", "T" * 31 + "A", "C" + "T" * 32, "G" * 32]
    ref = expect("acgt", 32, reads)
    n_a, n_t = occurrences_of("acgt", "A" * 32), occurrences_of("acgt", "T" * 32)
    assert n_a >= 200 - 31 and n_t == 70 - 31
    assert ref["window_counts"][0] == n_a and ref["window_counts"][32] == n_t
    assert ref["n_present"].tolist()[:3] == [1, 1, 2] and ref["n_present"][6] == 0
    check(monkeypatch, "acgt", 32, reads, ref=ref)
    both = expect("acgt", 32, reads, both=True)
    assert both["window_counts"][0] == n_a + n_t  # all-A plus its reverse complement, all-T
    check(monkeypatch, "acgt", 32, reads, both=True, ref=both)


def test_genome_of_2e5_bases(monkeypatch):
    reads = sample_reads("big", 7, 300, 150, n_every=11)
    ref = expect("big", 31, reads)
    assert screenref.nontrivial(ref)
    check(monkeypatch, "big", 31, reads, ref=ref)


# ---------------------------------------------------------------------------------------------
# 2. tile edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 12])
def test_tile_edge_sweep(K, monkeypatch):
    """A read boundary, a single N and the batch's end at every position T - K - 1 ... T + K + 1."""
    name = "acg" if K < 8 else "acgt"
    main = genome(name)[0][1]
    # substitutions about every 200 bases: some windows absent; the poly-A region keeps counts above 1
    long = mutate(main[11900:11900 + 3 * T], 3, every=200)
    for d in range(T - K - 1, T + K + 2):
        batches = {
            "boundary": [long[:d], main[2000:2000 + T]],
            "N": [long[:d] + "N" + long[d + 1:2 * T + 50]],
            "end": [long[:d]],
        }
        for what, reads in batches.items():
            ref = expect(name, K, reads)
            assert screenref.nontrivial(ref), (d, what)
            check(monkeypatch, name, K, reads, ref=ref, paths=("bytes", "keys"))


def test_read_across_more_than_three_tiles(monkeypatch):
    """Sums that cross blocks; the rolling key restarted in every thread's run."""
    K = 31
    main = genome("acgt")[0][1]
    reads = [main[50:57], main[9000:9000 + 3 * T + 700], main[100:100 + K], main[200:200 + K + WIN], "",
             mutate(main[15000:15000 + 4 * T + 1], 5, every=90), main[12100:12100 + K - 1]]
    ref = expect("acgt", K, reads)
    assert screenref.nontrivial(ref) and ref["n_windows"][1] > 3 * T
    assert ref["n_windows"].tolist()[2:4] == [1, WIN + 1]
    check(monkeypatch, "acgt", K, reads, ref=ref)
    check(monkeypatch, "acgt", K, reads, both=True)


@pytest.mark.parametrize("K", [3, 12])
def test_more_boundaries_than_the_lds_table(K, monkeypatch):
    """Hundreds of reads of length 0, 1, K - 1 and K in one tile: several passes over the tile."""
    name = "acg" if K < 8 else "acgt"
    main = genome(name)[0][1]
    reads, at = [main[11950:11950 + 300]], 0
    pattern = [0, 0, 0, 1, 0, K - 1, 0, 0, K, 0]
    sources = (main[:11000], "A" * 64, "TTGCA" * 13)
    for i in range(900):
        ln = pattern[i % len(pattern)]
        src = sources[i % 3]
        reads.append(src[at % (len(src) - K):at % (len(src) - K) + ln])
        at += 7
    reads += [""] * 700 + [main[12000:12000 + 2 * T]] + [""] * 300 + [main[500:500 + K], main[600:600 + K + WIN]]
    ref = expect(name, K, reads)
    off = ref["offsets"].astype(np.int64)
    per_tile = np.bincount(off[1:-1] // T)  # read boundaries per tile
    assert per_tile.max() > 2 * BOUNDS
    assert screenref.nontrivial(ref)
    check(monkeypatch, name, K, reads, ref=ref)
    check(monkeypatch, name, K, reads, both=True)


# ---------------------------------------------------------------------------------------------
# 3. chunk edges
# ---------------------------------------------------------------------------------------------
def test_many_chunks_equal_one_chunk(monkeypatch):
    K = 31
    reads = sample_reads("acgt", 3, 330, 150, n_every=9) + [genome("acgt")[0][1][11000:11500]]
    ref = expect("acgt", K, reads)
    assert int(ref["offsets"][-1]) == 50000 and screenref.nontrivial(ref)
    km = sorted_kmers("acgt", K)
    monkeypatch.delitem(_native.options, "GKM_SCREEN_CHUNK", raising=False)
    one = km.screen(reads, per_window=True)
    assert_equal(one, ref, "one chunk")
    for chunk in (4096, 4099, 1500, 150, 301, 97):
        monkeypatch.setitem(_native.options, "GKM_SCREEN_CHUNK", str(chunk))
        for path in ("keys", "bytes") if chunk >= 1500 else ("keys",):
            force(monkeypatch, path)
            res = km.screen(reads, per_window=True)
            assert_equal(res, ref, f"chunk {chunk} {path}")
            for out in OUTPUTS:
                np.testing.assert_array_equal(getattr(res, out), getattr(one, out))
        force(monkeypatch, "auto")
        assert_equal(km.screen(reads, both_strands=True, per_window=True), expect("acgt", K, reads, both=True),
                     f"chunk {chunk} both")


@pytest.mark.parametrize("K", [3, 12])
def test_chunk_edge_sweep(K, monkeypatch):
    """A read boundary across a chunk's end and through its K - 1 overlap; a chunk that ends exactly on
    a read's last byte (d == C) and one whose owned positions do (d == C - K + 1)."""
    C = 1024 + 77
    name = "acg" if K < 8 else "acgt"
    main = genome(name)[0][1]
    km = sorted_kmers(name, K)
    seen = set()
    for d in range(C - 2 * K - 1, C + K + 2):
        reads = [main[11800:11800 + d], main[4000:4000 + 2 * C], main[30:30 + K], rand_seq(5, 200), "A" * 40]
        ref = expect(name, K, reads)
        assert screenref.nontrivial(ref), d
        monkeypatch.delitem(_native.options, "GKM_SCREEN_CHUNK", raising=False)
        one = km.screen(reads, per_window=True)
        monkeypatch.setitem(_native.options, "GKM_SCREEN_CHUNK", str(C))
        for path in ("keys", "bytes"):
            force(monkeypatch, path)
            res = km.screen(reads, per_window=True)
            assert_equal(res, ref, f"d={d} {path}")
            np.testing.assert_array_equal(res.window_counts, one.window_counts)
        seen.add(d)
    assert C in seen and C - K + 1 in seen


def test_chunk_of_one_window(monkeypatch):
    """GKM_SCREEN_CHUNK below K is raised to K: every chunk owns one position."""
    K = 12
    main = genome("acgt")[0][1]
    reads = [main[11990:12100], "", main[5:5 + K], "ACGTN" * 6, main[700:700 + K - 1]]
    ref = expect("acgt", K, reads)
    monkeypatch.setitem(_native.options, "GKM_SCREEN_CHUNK", "5")
    check(monkeypatch, "acgt", K, reads, ref=ref)
    monkeypatch.setitem(_native.options, "GKM_SCREEN_CHUNK", str(K + 1))
    check(monkeypatch, "acgt", K, reads, ref=ref)


# ---------------------------------------------------------------------------------------------
# 4. the byte path's ground
# ---------------------------------------------------------------------------------------------
def refused_keys(monkeypatch, km, reads):
    force(monkeypatch, "keys")
    with pytest.raises(_native.GkError, match="GKM_SCREEN_PATH=keys") as e:
        km.screen(reads)
    assert e.value.code == _native.GK_E_UNSUPPORTED
    force(monkeypatch, "auto")


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [5, 31, 40])
def test_mixed_genome(K, both, monkeypatch):
    """N runs and IUPAC letters in the index: reads match byte for byte, N against N included."""
    contigs = dict(genome("mixed"))
    gold = contigs["gold_again"]
    npos = gold.find("N")
    assert npos >= 0
    lo = max(0, npos - 60)
    reads = sample_reads("mixed", 40 + K, 45, 120, n_every=5)
    reads += [gold[lo:lo + 200], contigs["r1"][550:700], contigs["r1"][3590:3640], "N" * 60, "", "RYKM" * 12,
              screenref.revcomp(contigs["r1"][560:690])]
    ref = expect("mixed", K, reads, both=both)
    assert screenref.nontrivial(ref)
    arr, off = screenref.pack(reads)
    starts = np.flatnonzero(ref["window_counts"] > 0)
    with_n = [p for p in starts.tolist() if b"N" in arr[p:p + K].tobytes()]
    assert with_n, "a present window that holds an N"
    ref, km = check(monkeypatch, "mixed", K, reads, both=both, ref=ref)
    refused_keys(monkeypatch, km, reads)


@pytest.mark.parametrize("K", [40, 63])
def test_long_kmers(K, monkeypatch):
    reads = sample_reads("acgt", 60 + K, 40, 150, n_every=6) + ["A" * 100, genome("acgt")[0][1][2990:3720]]
    ref = expect("acgt", K, reads)
    assert screenref.nontrivial(ref)
    ref, km = check(monkeypatch, "acgt", K, reads, ref=ref)
    refused_keys(monkeypatch, km, reads)
    check(monkeypatch, "acgt", K, reads, both=True)


@pytest.mark.parametrize("name,min_len,K", [("acgt", 10, 31), ("mixed", 6, 25), ("acgt", 1, 12)])
def test_min_below_max(name, min_len, K, monkeypatch):
    """An index that also holds k-mers cut short by a contig's end: they match no window of K bytes."""
    tail = genome(name)[-1][1]
    reads = sample_reads(name, 80 + K, 40, 100, n_every=8) + [tail[-K:], tail[-(K - 1):], tail[-(K + 5):], "A" * 60]
    ref = expect(name, K, reads)
    assert screenref.nontrivial(ref)
    ref, km = check(monkeypatch, name, K, reads, min_len=min_len, ref=ref)
    refused_keys(monkeypatch, km, reads)
    check(monkeypatch, name, K, reads, min_len=min_len, both=True)


@pytest.mark.parametrize("name", ["acgt", "mixed"])
@pytest.mark.parametrize("K", [21, 31])
def test_canonical_orders(name, K, monkeypatch):
    """The window is canonicalised on the device; the both-strands flag changes nothing."""
    reads = sample_reads(name, 90 + K, 60, 130, n_every=7) + ["A" * 50, "T" * 50, ""]
    ref = expect(name, K, reads, canonical=True)
    assert screenref.nontrivial(ref)
    ref, km = check(monkeypatch, name, K, reads, canonical=True, ref=ref)
    refused_keys(monkeypatch, km, reads)
    assert_equal(km.screen(reads, both_strands=True, per_window=True), ref, "flag on a canonical order")


def test_reads_with_n_on_an_acgt_index(monkeypatch):
    """Every window that holds an N counts 0, on both paths; its neighbours are not disturbed."""
    K = 12
    main = genome("acgt")[0][1]
    reads = []
    for i, p in enumerate(range(0, 60, 3)):
        r = main[1000 + 100 * i:1000 + 100 * i + 60]
        reads.append(r[:p] + "N" + r[p + 1:])
    reads += ["N" * K, "N", main[12000:12050] + "NN" + main[12052:12100], "R" + main[100:140] + "Y"]
    ref = expect("acgt", K, reads)
    arr, off = screenref.pack(reads)
    for p in np.flatnonzero(arr == ord("N")).tolist():
        assert not ref["window_counts"][max(0, p - K + 1):p + 1].any()
    assert screenref.nontrivial(ref)
    check(monkeypatch, "acgt", K, reads, ref=ref)


# ---------------------------------------------------------------------------------------------
# 5. strands
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("acgt", 12), ("acgt", 31), ("mixed", 21), ("acgt", 40)])
def test_both_strands_equals_canonical(name, K, monkeypatch):
    main = genome(name)[-2][1] if name == "mixed" else genome(name)[0][1]
    reads = [screenref.revcomp(main[300:520]), main[300:520], screenref.revcomp(mutate(main[2000:2300], 3)),
             rand_seq(77, 200), "A" * 40, "T" * 40, PALINDROME * 3, ""]
    plain = expect(name, K, reads)
    both = expect(name, K, reads, both=True)
    canon = expect(name, K, reads, canonical=True)
    assert screenref.nontrivial(both)
    assert plain["n_present"][0] == 0 and both["n_present"][0] == both["n_windows"][0]  # reverse-strand read
    for out in OUTPUTS:
        np.testing.assert_array_equal(both[out], canon[out])
    check(monkeypatch, name, K, reads, ref=plain)
    check(monkeypatch, name, K, reads, both=True, ref=both)
    check(monkeypatch, name, K, reads, canonical=True, ref=canon)


def test_even_k_palindrome_counts_once(monkeypatch):
    K = 12
    reads = [PALINDROME, "C" + PALINDROME + "G", screenref.revcomp(PALINDROME)]
    plain = expect("acgt", K, reads)
    both = expect("acgt", K, reads, both=True)
    n = int(plain["window_counts"][0])
    assert n >= 2 and both["window_counts"][0] == n  # not 2 n
    assert both["window_counts"][K + 1] == n and both["window_counts"][2 * K + 2] == n
    check(monkeypatch, "acgt", K, reads, ref=plain)
    check(monkeypatch, "acgt", K, reads, both=True, ref=both)


# ---------------------------------------------------------------------------------------------
# 6. cross-check with Kmers.find
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,canonical", [("acgt", 31, False), ("mixed", 21, True)])
def test_window_counts_equal_find(name, K, canonical, monkeypatch):
    reads = sample_reads(name, 5, 30, 120, n_every=4) + ["A" * 45, ""]
    ref = expect(name, K, reads, canonical=canonical)
    assert screenref.nontrivial(ref)
    ref, km = check(monkeypatch, name, K, reads, canonical=canonical, ref=ref)
    res = km.screen(reads, per_window=True)
    arr, off = _native.pack_sequences(reads)
    starts = np.concatenate([np.arange(int(a), int(b) - K + 1) for a, b in zip(off[:-1], off[1:]) if b - a >= K])
    windows = np.lib.stride_tricks.sliding_window_view(arr, K)[starts]
    _, count = km.find(np.ascontiguousarray(windows))
    np.testing.assert_array_equal(res.window_counts[starts], count)
    rest = np.ones(arr.size, dtype=bool)
    rest[starts] = False
    assert not res.window_counts[rest].any()


# ---------------------------------------------------------------------------------------------
# 7. preconditions and lifetime
# ---------------------------------------------------------------------------------------------
def fresh_kmers(K, max_len="K", sort=False):
    sc = SequenceCollection(sequence_list=[("c", rand_seq(1, 500))], strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K, max_kmer_len=K if max_len == "K" else max_len)
    if sort:
        km.sort()
    return km


def raw_screen(km, arr, off, flags=0, null_seqs=False):
    """gk_screen through the C binding with the arrays as given (no pack_sequences)."""
    import ctypes

    km._sync_device()
    eng = km._get_engine()
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    nseq = off.size - 1
    n_present = np.zeros(max(nseq, 1), dtype=np.uint32)
    occ = np.zeros(max(nseq, 1), dtype=np.uint64)
    rc = eng.lib.gk_screen(eng.ctx, None if null_seqs else _native._ptr(arr, ctypes.c_uint8),
                           _native._ptr(off, ctypes.c_uint64), nseq, flags, _native._ptr(n_present, ctypes.c_uint32),
                           _native._ptr(occ, ctypes.c_uint64), None)
    msg = eng.lib.gk_last_error(eng.ctx)
    return rc, (msg.decode() if msg else ""), n_present, occ


def test_preconditions():
    reads = ["ACGTACGTACGT"]
    arr, off = _native.pack_sequences(reads)
    km = fresh_kmers(5)
    with pytest.raises(AssertionError, match="must be sorted when calling screen"):
        km.screen(reads)
    rc, msg, _, _ = raw_screen(km, arr, off)
    assert rc == _native.GK_E_STATE and "not sorted" in msg
    none = fresh_kmers(2, max_len=None, sort=True)
    with pytest.raises(ValueError, match="max_kmer_len is None"):
        none.screen(reads)
    rc, msg, _, _ = raw_screen(none, arr, off)
    assert rc == _native.GK_E_UNSUPPORTED and "fixed max_kmer_len" in msg
    km = fresh_kmers(5, sort=True)
    for bad_off, what in (([1, 12], "offsets\\[0\\] must be 0"), ([0, 8, 4, 12], "offsets decrease at sequence 1")):
        with pytest.raises(_native.GkError, match=what) as e:
            km._engine.screen(arr, np.array(bad_off, dtype=np.uint64))
        assert e.value.code == _native.GK_E_ARG
    with pytest.raises(ValueError, match="offsets must"):
        km.screen((arr, np.array([0, 8, 4, 12], dtype=np.uint64)))
    # an over-long sequence: refused from the offsets alone, before any byte is read (there are none)
    rc, msg, _, _ = raw_screen(km, arr, [0, 1 << 32], null_seqs=True)
    assert rc == _native.GK_E_ARG and "sequence 0 is longer than 2^32 - 1 bytes" in msg
    rc, msg, _, _ = raw_screen(km, arr, [0, 3, 3 + (1 << 32)], null_seqs=True)
    assert rc == _native.GK_E_ARG and "sequence 1 is longer" in msg
    rc, msg, _, _ = raw_screen(km, arr, off, flags=2)
    assert rc == _native.GK_E_ARG and "flag" in msg
    rc, msg, _, _ = raw_screen(km, arr, off, null_seqs=True)
    assert rc == _native.GK_E_ARG and "null" in msg


def test_path_knob_values(monkeypatch):
    km = sorted_kmers("acgt", 12)
    monkeypatch.setitem(_native.options, "GKM_SCREEN_PATH", "key")
    with pytest.raises(_native.GkError, match="GKM_SCREEN_PATH must be 'bytes' or 'keys'") as e:
        km.screen("ACGTACGTACGTACGT")
    assert e.value.code == _native.GK_E_ARG


@pytest.mark.parametrize("path", ["bytes", "keys"])
def test_bytes_outside_the_alphabet(path, monkeypatch):
    """Lower case and '$', found on the device: the message names sequence and offset, also when the
    byte lies in a later chunk or in a read's last K - 1 bytes, where no window starts."""
    K = 12
    km = sorted_kmers("acgt", K)
    main = genome("acgt")[0][1]
    reads = [main[100:400], "", main[500:800], main[900:1500]]
    arr, off = _native.pack_sequences(reads)
    force(monkeypatch, path)
    for chunk in (None, 256):
        if chunk:
            monkeypatch.setitem(_native.options, "GKM_SCREEN_CHUNK", str(chunk))
        for seq, at, byte in ((0, 0, "a"), (2, 17, "$"), (3, 599, "c"), (3, 300, "X"), (2, 299, "n")):
            bad = arr.copy()
            bad[int(off[seq]) + at] = ord(byte)
            want = re.escape(f"sequence {seq} holds byte 0x{ord(byte):02x} ('{byte}') at offset {at},")
            with pytest.raises(_native.GkError, match=want) as e:
                km._engine.screen(bad, off)
            assert e.value.code == _native.GK_E_ALPHABET
        two = arr.copy()  # the first bad byte is the one named
        two[int(off[3]) + 5] = ord("x")
        two[int(off[2]) + 250] = ord("y")
        with pytest.raises(_native.GkError, match="sequence 2 holds byte 0x79 .* at offset 250,"):
            km._engine.screen(two, off)
        # the context serves the next call
        assert_equal(km.screen(reads, per_window=True), expect("acgt", K, reads), "after an error")
    with pytest.raises(ValueError, match="sequence 1 holds the character 'a' at offset 1"):
        km.screen(["ACGT", "CaT"])


def test_empty_batches(monkeypatch):
    km = sorted_kmers("acgt", 12)
    for path in ("auto", "bytes", "keys"):
        force(monkeypatch, path)
        res = km.screen([], per_window=True)
        assert all(len(getattr(res, out)) == 0 for out in OUTPUTS[:4]) and res.offsets.tolist() == [0]
        res = km.screen(["", "", ""], per_window=True)
        assert res.n_windows.tolist() == [0, 0, 0] and res.n_present.tolist() == [0, 0, 0]
        assert res.occurrences.tolist() == [0, 0, 0] and len(res.window_counts) == 0
        res = km.screen("")
        assert res.n_windows.tolist() == [0] and res.occurrences.tolist() == [0]
        res = km.screen(["ACGTACGTACG", "A", ""])  # every read shorter than K
        assert res.n_windows.tolist() == [0, 0, 0] and res.occurrences.tolist() == [0, 0, 0]
    # the C call writes zeros over whatever the arrays held
    rc, _, n_present, occ = raw_screen(km, np.zeros(0, dtype=np.uint8), [0, 0, 0])
    assert rc == _native.GK_OK and not n_present.any() and not occ.any()


def test_single_str_is_a_batch_of_one(monkeypatch):
    km = sorted_kmers("acgt", 12)
    main = genome("acgt")[0][1]
    res = km.screen(main[100:160], per_window=True)
    ref = expect("acgt", 12, [main[100:160]])
    assert_equal(res, ref)
    assert res.n_windows.tolist() == [49] and res.n_present.tolist() == [49]
    assert_equal(km.screen(main[100:160].encode(), per_window=True), ref)
    assert_equal(km.screen(_native.pack_sequences([main[100:160]]), per_window=True), ref)


def test_screen_disturbs_nothing(monkeypatch):
    """find, get_unique_kmers and count_in give the same after a screen as before."""
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
        assert_equal(km.screen(reads, per_window=True), ref, path)
        first, count = km._engine.join_result()  # the join result is still there
        np.testing.assert_array_equal(first, before[2][0])
        np.testing.assert_array_equal(count, before[2][1])
        after = (km.find(queries), km.get_unique_kmers(), km.count_in(other), km.kmer_sba_start_indices)
        for b, a in zip(before[:3], after[:3]):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(after[3], before[3])
        assert_equal(km.screen(reads, per_window=True), ref, path + " again")


@pytest.mark.parametrize("name,K", [("acgt", 12), ("mixed", 21)])
def test_after_reference_order_sorts(name, K, monkeypatch):
    reads = sample_reads(name, 13, 40, 120, n_every=6) + ["A" * 40]
    ref = expect(name, K, reads)
    assert screenref.nontrivial(ref)
    km = sorted_kmers(name, K, order="reference")
    for path in ("auto", "bytes"):
        force(monkeypatch, path)
        assert_equal(km.screen(reads, per_window=True), ref, path)
        assert_equal(km.screen(reads, both_strands=True, per_window=True), expect(name, K, reads, both=True), path)
