"""tests/matchref.py (the numpy reference of gk_match that the GPU tests trust) pinned to a pure-Python
brute force -- ``any(s.startswith(...))`` over the k-mers as a list of bytes -- on genomes of a few
hundred bases: bounded sorts, min < max, max_kmer_len None with a cap, contig ends, 'N' in reads and in
the genome, empty reads, reads shorter than the cap, an index of one k-mer.  And the pure function
``kmers.maximal_from_lengths`` against a hand-written loop.  No GPU."""

import numpy as np
import pytest

import matchref
from genome_kmers import kmers as gk
from genome_kmers.kmers import MatchResult, maximal_from_lengths  # noqa: F401  (the feature under test)


def rand_seq(seed, n, letters="ACGT") -> str:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters.encode(), dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


def small_genome(letters="ACGT"):
    a = rand_seq(1, 180, letters)
    return [("c0", a), ("c1", a[40:75] + rand_seq(2, 60, letters)), ("short", "ACG"), ("polyA", "A" * 25),
            ("c2", rand_seq(3, 40, letters) + a[100:130])]


def small_reads(genome, seed, with_n=False):
    rng = np.random.default_rng(seed)
    src = genome[0][1]
    reads = ["", src[5:60], src[170:180] + "T", rand_seq(seed + 10, 50), src[50:52], "A" * 30, "",
             genome[1][1][30:40] + genome[4][1][:12], src[-20:] + genome[1][1][:20], "G"]
    s = bytearray(src[90:150].encode())
    for p in rng.integers(0, len(s), 3).tolist():
        s[p] = ord("ACGT"[("ACGT".index(chr(s[p])) + 1) % 4]) if chr(s[p]) in "ACGT" else ord("A")
    reads.append(s.decode())
    if with_n:
        reads += [src[5:25] + "N" + src[26:50], "NNNN", genome[0][1][60:75]]
    return reads


CASES = [
    # (letters, min_len, max_len, cap, reads with N)
    ("ACGT", 12, 12, 12, True),
    ("ACGT", 3, 3, 3, False),
    ("ACGT", 31, 31, 31, True),
    ("ACGT", 12, 12, 5, False),        # a cap below K
    ("ACGT", 4, 12, 12, True),         # k-mers cut short by contig ends
    ("ACGT", 1, 20, 20, False),
    ("ACGT", 5, None, 12, True),       # the suffix order with a cap
    ("ACGT", 1, None, 40, False),
    ("ACGTN", 8, 8, 8, True),          # N in the genome matches N in a read
    ("ACGTN", 2, None, 17, True),
]


@pytest.mark.parametrize("letters,min_len,max_len,cap,with_n", CASES)
def test_reference_equals_brute_force(letters, min_len, max_len, cap, with_n):
    genome = small_genome(letters)
    reads = small_reads(genome, 7, with_n)
    index = matchref.Index(matchref.as_sba(genome), min_len, max_len, cap)
    ref = matchref.match(index, reads)
    want = matchref.brute(genome, min_len, max_len, reads, cap)
    for out in ("lengths", "first", "count", "longest", "longest_pos", "sum_len"):
        np.testing.assert_array_equal(ref[out].astype(np.int64), want[out], err_msg=out)
    # not trivial: matches at the cap, no match at all, matches strictly between, a count above 1
    v = ref["lengths"]
    assert (v == cap).any()
    if with_n and letters == "ACGT":
        assert (v == 0).any()
    assert ((v > 0) & (v < cap)).any() and (ref["count"] > 1).any()
    assert index.n == sum(max(0, len(s) - min_len + 1) for _, s in genome)
    if min_len != max_len:  # some indexed k-mer is cut short by its contig's end
        assert (index.lens < cap).any()


def test_neighbour_sides_follow_the_insertion_point():
    genome = small_genome()
    reads = small_reads(genome, 9, True)
    index = matchref.Index(matchref.as_sba(genome), 12, 12, 12)
    ref = matchref.match(index, reads)
    sides = matchref.neighbour_sides(index, reads)
    assert ((sides > 0) == (ref["lengths"] > 0)).all()
    for side in (matchref.PREV, matchref.NEXT, matchref.PREV | matchref.NEXT):
        assert (sides == side).any()


def test_index_of_one_kmer():
    index = matchref.Index(matchref.as_sba("ACGTAC"), 6, 6, 6)
    assert index.n == 1
    reads = ["ACGTAC", "ACGTTT", "TTTT", "AAC", "CGTACGTAC", ""]
    ref = matchref.match(index, reads)
    want = matchref.brute("ACGTAC", 6, 6, reads, 6)
    for out in ("lengths", "first", "count", "longest", "longest_pos", "sum_len"):
        np.testing.assert_array_equal(ref[out].astype(np.int64), want[out], err_msg=out)
    assert ref["lengths"][:6].tolist() == [6, 0, 0, 0, 2, 0] and ref["longest"].tolist() == [6, 4, 0, 2, 6, 0]
    assert ref["longest_pos"].tolist() == [0, 0, 0, 1, 3, 0]


def test_empty_batches():
    index = matchref.Index(matchref.as_sba("ACGTACGTTT"), 4, 4, 4)
    ref = matchref.match(index, ["", "", ""])
    assert ref["lengths"].size == 0 and ref["longest"].tolist() == [0, 0, 0] and ref["sum_len"].tolist() == [0, 0, 0]
    ref = matchref.match(index, [])
    assert ref["offsets"].tolist() == [0] and ref["longest"].size == 0


@pytest.mark.parametrize("seed", range(6))
def test_maximal_from_lengths_equals_the_loop(seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, 12).tolist() + [0, 0, 1]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(offsets[-1])
    # runs that descend by one (the tails of one match) between random values
    v = rng.integers(0, 7, total)
    for p in range(1, total):
        if rng.integers(0, 2):
            v[p] = max(int(v[p - 1]) - 1, 0)
    v = v.astype(np.uint32)
    for min_len in (1, 2, 4, 7):
        read, pos, length = gk.maximal_from_lengths(v, offsets, min_len)
        want = matchref.maximal(v, offsets, min_len)
        assert read.dtype == np.int64 and pos.dtype == np.int64 and length.dtype == np.uint32
        np.testing.assert_array_equal(read, want[0])
        np.testing.assert_array_equal(pos, want[1])
        np.testing.assert_array_equal(length, want[2])
    assert len(gk.maximal_from_lengths(v, offsets, 1)[0]) > 0


def test_maximal_from_lengths_by_hand():
    #          read 0          | read 1   | read 2 (empty) | read 3
    v = np.array([5, 4, 3, 5, 0, 3, 2, 1,                    2, 2], dtype=np.uint32)
    offsets = np.array([0, 5, 8, 8, 10])
    read, pos, length = gk.maximal_from_lengths(v, offsets, 2)
    assert read.tolist() == [0, 0, 1, 3, 3] and pos.tolist() == [0, 3, 0, 0, 1] and length.tolist() == [5, 5, 3, 2, 2]
    read, pos, length = gk.maximal_from_lengths(v, offsets, 6)
    assert read.size == 0 and pos.size == 0 and length.size == 0
    empty = gk.maximal_from_lengths(np.zeros(0, dtype=np.uint32), np.array([0, 0]), 1)
    assert all(a.size == 0 for a in empty)
    with pytest.raises(ValueError, match="maximal_from_lengths takes"):
        gk.maximal_from_lengths(v, offsets[:-1], 2)
