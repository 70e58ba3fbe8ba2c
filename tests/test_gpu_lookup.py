"""Batch k-mer lookup on the device: gk_lookup through Kmers.find / count / in / get_kmer_locations and
_native.Engine.lookup, on both paths (bytes, keys).

The expected values never come from the code under test.  From the host sba and a sorted start array
(the reference's golden ``starts_stable``, or a host sort of the enumeration for synthetic genomes),
``t[i] = bytes(sba[s:s+q]).split(b"$")[0]`` is the k-mer at sorted position i cut at its contig's end;
Python's bytes order -- a proper prefix is smaller -- is the reference comparator's order
(compare_sba_kmers_lexicographically, kmers.py:306-397), so ``first = bisect_left(t, query)`` and
``count = bisect_right(t, query) - first``.
"""

from bisect import bisect_left, bisect_right
from functools import lru_cache

import numpy as np
import pytest

from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection
from oracle import oracle

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in load_manifest()}
# Test 1's cases: one fixed length, min_kmer_len == max_kmer_len.  A case with min < max also has a
# fixed max_kmer_len, but there a present k-mer shorter than max (one that meets its contig's end) is a
# prefix query: its range covers every k-mer that starts with it, not its own get_unique_kmers()
# group, so the two cannot be compared.  Those cases are test_variable_length_and_none's.
FIXED = [c for c in CASES.values() if c["max_kmer_len"] is not None and c["min_kmer_len"] == c["max_kmer_len"]]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# host expectations
# ---------------------------------------------------------------------------------------------
def cut_kmers(sba, sorted_starts, q):
    """t[i]: the q bytes at sorted start i, cut at the '$' / the end of the sba."""
    raw = bytes(np.asarray(sba, dtype=np.uint8))
    return [raw[s:s + q].split(b"$")[0] for s in np.asarray(sorted_starts).tolist()]


def expect(t, queries):
    first = np.array([bisect_left(t, x) for x in queries], dtype=np.uint64)
    count = np.array([bisect_right(t, x) for x in queries], dtype=np.uint64) - first
    return first, count.astype(np.uint32)


def host_sorted(sba, starts, K):
    """The stable order (k-mer cut at K, then start) of the given starts, sorted on the host."""
    raw = bytes(np.asarray(sba, dtype=np.uint8))
    pairs = sorted((raw[s:s + K].split(b"$")[0] if K else raw[s:].split(b"$")[0], s) for s in starts.tolist())
    return np.array([s for _, s in pairs], dtype=np.uint32)


@lru_cache(maxsize=None)
def golden(name):
    case = CASES[name]
    a = load_case(name)
    for v in a.values():
        v.setflags(write=False)
    return case, a


@lru_cache(maxsize=None)
def golden_t(name, q):
    _, a = golden(name)
    return cut_kmers(a["sba"], a["starts_stable"], q)


def sorted_kmers(name):
    case, a = golden(name)
    sc = SequenceCollection(sequence_list=seq_list_of(case, a), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=case["min_kmer_len"], max_kmer_len=case["max_kmer_len"])
    km.sort()
    return km


def kmers_of(seqs, kmin, kmax):
    sc = SequenceCollection(sequence_list=seqs, strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=kmin, max_kmer_len=kmax)
    unsorted = km.kmer_sba_start_indices.copy()
    return sc, km, unsorted


def keys_valid(case, a):
    """The key path serves the case: ACGT-only sba, one fixed length of at most 32 bases."""
    return (case["min_kmer_len"] == case["max_kmer_len"] and case["max_kmer_len"] <= 32
            and bool(np.isin(a["sba"], np.frombuffer(b"ACGT$", dtype=np.uint8)).all()))


def check(km, t, queries):
    """find(queries) equals the bisect values over t; returns the expected counts."""
    first, count = expect(t, queries)
    got_first, got_count = km.find(queries)
    assert got_first.dtype == np.uint64 and got_count.dtype == np.uint32
    np.testing.assert_array_equal(got_count, count)
    np.testing.assert_array_equal(got_first, first)
    return count


def random_acgt(rng, m, q):
    return [bytes(r) for r in ACGT[rng.integers(0, 4, (m, q))]]


def mutate_last(kmers):
    """every k-mer with its last base changed (A->C->G->T->A; other letters -> A)"""
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    return [x[:-1] + bytes([nxt.get(x[-1], 65)]) for x in kmers]


PATHS = ["auto", "bytes", "keys"]


def case_paths(names):
    """(case, path) pairs: the key path only where it serves the case"""
    return [(n, p) for n in names for p in PATHS if p != "keys" or keys_valid(*golden(n))]


def force(monkeypatch, path):
    if path != "auto":
        monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", path)


# ---------------------------------------------------------------------------------------------
# 1. golden cases, every present k-mer
# ---------------------------------------------------------------------------------------------
# (the refusal of a forced key path where it does not serve is test_mixed_alphabet's)
@pytest.mark.parametrize("name,path", case_paths([c["name"] for c in FIXED]))
def test_present_kmers_equal_unique_groups(name, path, monkeypatch):
    case, a = golden(name)
    force(monkeypatch, path)
    K = case["max_kmer_len"]
    t = golden_t(name, K)
    km = sorted_kmers(name)
    group_start, group_count = km.get_unique_kmers()
    distinct = sorted(set(t))
    assert len(distinct) == len(group_start)
    first, count = km.find(distinct)
    np.testing.assert_array_equal(first, group_start)
    np.testing.assert_array_equal(count, group_count)
    check(km, t, distinct)


# ---------------------------------------------------------------------------------------------
# 2. absent k-mers and insertion points
# ---------------------------------------------------------------------------------------------
# (K >= 21: 4^K far above the k-mer count, so random strings and single-base changes are mostly absent;
# the present k-mers themselves are queried beside them so that both sides hold at least 30 %)
ABSENT_CASES = ["rand10k_k31", "repeat_k31", "repeat_k40", "iupac_k31"]


@pytest.mark.parametrize("name,path", case_paths(ABSENT_CASES))
def test_absent_kmers_insertion_points(name, path, monkeypatch):
    case, a = golden(name)
    force(monkeypatch, path)
    K = case["max_kmer_len"]
    t = golden_t(name, K)
    present = sorted(set(t))
    rng = np.random.default_rng(len(name) * 1000 + K)
    queries = random_acgt(rng, 1000, K) + mutate_last(present) + present
    _, want = expect(t, queries)
    assert (want == 0).mean() >= 0.3 and (want > 0).mean() >= 0.3
    check(sorted_kmers(name), t, queries)


# ---------------------------------------------------------------------------------------------
# 3. prefix queries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["c1_seed42_10kb_k5", "rand10k_k31"])
def test_prefix_queries(name, path, monkeypatch):
    force(monkeypatch, path)
    case, a = golden(name)
    K = case["max_kmer_len"]
    km = sorted_kmers(name)
    rng = np.random.default_rng(K)
    for q in (1, 2, K - 1, K):
        t = golden_t(name, q)
        queries = sorted(set(t)) + random_acgt(rng, 200, q)
        if q == 1:
            queries = [b"A", b"C", b"G", b"T"]
        count = check(km, t, queries)
        if q == 1:  # the base counts of the k-mer starts
            sba = a["sba"]
            want = [int((sba[a["starts_stable"]] == b).sum()) for b in b"ACGT"]
            assert count.tolist() == want and sum(want) == len(t)


# ---------------------------------------------------------------------------------------------
# 4. word edges: key 0, key all ones, K = 32 (shift 0) and K = 31
# ---------------------------------------------------------------------------------------------
def word_edge_genome():
    rng = np.random.default_rng(41)
    seqs = []
    for i, L in enumerate((11_000, 9_000)):
        s = ACGT[rng.integers(0, 4, L)].copy()
        s[500:540] = ord("T")
        s[3000:3040] = ord("A")
        s[6000:6040] = np.frombuffer(b"ACGT" * 10, dtype=np.uint8)
        if i == 1:  # runs at a contig's start and end as well
            s[:40] = ord("A")
            s[-40:] = ord("T")
        seqs.append((f"c{i}", s.tobytes().decode()))
    return seqs


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("K", [32, 31])
def test_word_edges(K, path, monkeypatch):
    force(monkeypatch, path)
    sc, km, unsorted = kmers_of(word_edge_genome(), K, K)
    order = host_sorted(sc.forward_sba, unsorted, K)
    km.sort()
    np.testing.assert_array_equal(km.kmer_sba_start_indices, order)
    t = cut_kmers(sc.forward_sba, order, K)
    T, A, R = b"T" * K, b"A" * K, (b"ACGT" * 10)[:K]
    queries = [T, A, R, (b"CGTA" * 10)[:K], T[:-1] + b"G", b"G" + T[1:], A[:-1] + b"C", b"C" + A[1:],
               T[:-1] + b"A", A[:-1] + b"T", b"T" + A[1:], b"A" + T[1:], R[:-1] + b"A", R[:-1] + b"T"]
    count = check(km, t, queries)
    assert count[0] >= 3 * (40 - K + 1) and count[1] >= 3 * (40 - K + 1) and count[2] >= 2
    for q in (1, 5, 11, 12, K - 1):  # (2 q below, at and above the directory's 22 bits)
        tq = cut_kmers(sc.forward_sba, order, q)
        check(km, tq, [b"T" * q, b"A" * q, b"G" * q, (b"ACGT" * 10)[:q], b"T" * (q - 1) + b"A"])
    check(km, cut_kmers(sc.forward_sba, order, 1), [b"A", b"C", b"G", b"T"])


# ---------------------------------------------------------------------------------------------
# 5. dense buckets: a two-letter genome, long shared prefixes; chunked launches
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(5)
    K = 31
    s = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, 200_000)]
    sc, km, unsorted = kmers_of([("ac", s.tobytes().decode())], K, K)
    order = host_sorted(sc.forward_sba, unsorted, K)
    t = cut_kmers(sc.forward_sba, order, K)
    present = [t[i] for i in rng.integers(0, len(t), 2000)]
    absent = [bytes(r) for r in np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, (2000, K))]]
    queries = present + absent
    first, count = expect(t, queries)
    assert (count[:2000] > 0).all() and (count[2000:] == 0).mean() > 0.95
    km.sort()
    return km, queries, first, count


@pytest.mark.parametrize("chunk", [None, "1500", "700"])
@pytest.mark.parametrize("path", PATHS)
def test_dense_buckets(dense, path, chunk, monkeypatch):
    force(monkeypatch, path)
    if chunk:  # 4,000 queries in launches of 1,500 (three, the last one partial) or 700 (six: both staging slots reused)
        monkeypatch.setitem(_native.options, "GKM_LOOKUP_CHUNK", chunk)
    km, queries, first, count = dense
    got_first, got_count = km.find(queries)
    np.testing.assert_array_equal(got_count, count)
    np.testing.assert_array_equal(got_first, first)


def test_directory_off_gives_the_same(dense, monkeypatch):
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", "keys")
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_DIR", "0")
    km, queries, first, count = dense
    got_first, got_count = km.find(queries)
    np.testing.assert_array_equal(got_count, count)
    np.testing.assert_array_equal(got_first, first)


# ---------------------------------------------------------------------------------------------
# 6. contig ends
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "bytes"])
def test_contig_ends(path, monkeypatch):
    force(monkeypatch, path)
    K = 6
    rng = np.random.default_rng(66)
    contigs = [bytes(ACGT[rng.integers(0, 4, L)]) for L in (60, 45, 70)]
    # min_kmer_len 1: the last K - 1 starts of every contig are k-mers too (shorter than K)
    sc, km, unsorted = kmers_of([(f"c{i}", c.decode()) for i, c in enumerate(contigs)], 1, K)
    sba = sc.forward_sba
    order = host_sorted(sba, unsorted, K)
    km.sort()
    np.testing.assert_array_equal(km.kmer_sba_start_indices, order)
    t = cut_kmers(sba, order, K)
    junctions = [contigs[i][-3:] + contigs[i + 1][:3] for i in range(2)]
    tails = [c[-j:] + b"A" * (K - j) for c in contigs for j in range(1, K)]  # a contig's tail, padded to K
    inside = [c[j:j + K] for c in contigs for j in (0, 7, len(c) - K)]
    queries = junctions + tails + inside
    first, count = expect(t, queries)
    assert (count[:2] == 0).all(), "the junction strings must not occur inside a contig (choose other contigs)"
    assert (count[-len(inside):] > 0).all()
    got_first, got_count = km.find(queries)
    np.testing.assert_array_equal(got_count, count)
    np.testing.assert_array_equal(got_first, first)
    # no match is one of the last K - 1 starts of a contig
    seg = np.append(sc._forward_sba_seg_starts.astype(np.int64), len(sba) + 1)
    last = np.concatenate([np.arange(e - 1 - (K - 1), e - 1) for e in seg[1:]])
    for f, c in zip(got_first.tolist(), got_count.tolist()):
        assert not np.isin(order[f:f + c], last).any()


# ---------------------------------------------------------------------------------------------
# 7. mixed alphabet
# ---------------------------------------------------------------------------------------------
def mixed_genome():
    """two contigs with N runs and planted repeats (test_gpu_configs' genome at a tenth of its size)"""
    rng = np.random.default_rng(12)
    rep = ACGT[rng.integers(0, 4, 300)]
    seqs = []
    for i, L in enumerate((70_000, 20_000)):
        s = ACGT[rng.integers(0, 4, L)].copy()
        for _ in range(12):
            at = int(rng.integers(0, L - 300))
            s[at:at + 300] = rep
        for _ in range(5):
            at = int(rng.integers(0, L - 500))
            s[at:at + int(rng.integers(40, 500))] = ord("N")
        seqs.append((f"c{i}", s.tobytes().decode()))
    return seqs


@pytest.mark.parametrize("path", ["auto", "bytes"])
def test_mixed_alphabet(path, monkeypatch):
    force(monkeypatch, path)
    K = 31
    sc, km, unsorted = kmers_of(mixed_genome(), K, K)
    sba = sc.forward_sba
    order = host_sorted(sba, unsorted, K)
    km.sort()
    np.testing.assert_array_equal(km.kmer_sba_start_indices, order)
    t = cut_kmers(sba, order, K)
    rng = np.random.default_rng(7)
    n_at = np.flatnonzero((sba[1:] == ord("N")) != (sba[:-1] == ord("N")))  # N-run edges
    raw = bytes(sba)
    straddle = [raw[p - j:p - j + K] for p in n_at.tolist() for j in (1, 15, 30)
                if p - j >= 0 and b"$" not in raw[p - j:p - j + K] and len(raw[p - j:p - j + K]) == K]
    acgt_present = [x for x in (t[i] for i in rng.integers(0, len(t), 500)) if set(x) <= set(b"ACGT")]
    queries = acgt_present + random_acgt(rng, 300, K) + [b"N" * K, b"N" * (K - 1) + b"A", b"A" + b"N" * (K - 1)] \
        + straddle
    assert len(straddle) >= 10 and len(acgt_present) >= 100
    count = check(km, t, queries)
    assert count[len(acgt_present) + 300] > 0  # N x K is present (runs of 40 and more)
    for q in (1, 4, 30):
        tq = cut_kmers(sba, order, q)
        check(km, tq, sorted(set(tq))[:300] + [b"N" * q, b"Y" * q, b"B" * q])
    # a forced key path is refused: the context holds 4-bit keys
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", "keys")
    with pytest.raises(_native.GkError) as e:
        km.find(acgt_present[:5])
    assert e.value.code == _native.GK_E_UNSUPPORTED
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", "bytes")
    check(km, t, acgt_present[:5])


def test_iupac_golden_case():
    name = "iupac_k31"
    km = sorted_kmers(name)
    for q in (1, 2, 17, 31):
        t = golden_t(name, q)
        check(km, t, sorted(set(t)) + [b"N" * q, b"A" * q])


# ---------------------------------------------------------------------------------------------
# 8. variable length and None (byte path)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "bytes"])
@pytest.mark.parametrize("name,qs", [("repeat_min10_max40", (1, 10, 25, 40)), ("iupac_min6_max25", (1, 6, 25)),
                                     ("seq2_min2_maxNone", (1, 3, 12, 40)), ("repeat_suffix_min4", (1, 3, 12, 40)),
                                     ("iupac_suffix_min2", (1, 3, 12, 40))])
def test_variable_length_and_none(name, qs, path, monkeypatch):
    force(monkeypatch, path)
    case, a = golden(name)
    km = sorted_kmers(name)
    rng = np.random.default_rng(8)
    for q in qs:
        t = golden_t(name, q)
        full = sorted({x for x in t if len(x) == q})
        short = sorted({x for x in t if len(x) < q})
        # k-mers that meet their contig's end before q bases, padded to q: never a match
        padded = [x + b"A" * (q - len(x)) for x in short[:200]] + [x + b"T" * (q - len(x)) for x in short[:200]]
        check(km, t, full + mutate_last(full) + padded + random_acgt(rng, 100, q))
    if case["max_kmer_len"] is None:
        assert any(len(x) < 40 for x in golden_t(name, 40)), "q = 40 must exceed some contigs"
    else:
        with pytest.raises(ValueError, match="more than max_kmer_len"):
            km.find("A" * (case["max_kmer_len"] + 1))
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", "keys")
    with pytest.raises(_native.GkError) as e:
        km.find("ACGT"[:min(qs[1], 4)])
    assert e.value.code == _native.GK_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# 9. canonical orders
# ---------------------------------------------------------------------------------------------
def revcomp(x: bytes) -> bytes:
    return bytes(oracle.reverse_complement(np.frombuffer(x, dtype=np.uint8)))


def canonical_genome(K, iupac):
    rng = np.random.default_rng(900 + K)
    s = ACGT[rng.integers(0, 4, 20_000)].copy()
    s[15_000:15_400] = oracle.reverse_complement(s[2000:2400])  # both strands of one stretch
    s[17_000:17_200] = s[3000:3200]
    if K % 2 == 0:  # a reverse palindrome of length K, twice
        h = ACGT[rng.integers(0, 4, K // 2)]
        pal = np.concatenate([h, oracle.reverse_complement(h)])
        s[8000:8000 + K] = pal
        s[9000:9000 + K] = pal
    if iupac:
        s[5000:5060] = ord("N")
        s[6000:6040:5] = ord("R")
        s[6500:6540:5] = ord("Y")
    cut = 12_000
    return [("c0", s[:cut].tobytes().decode()), ("c1", s[cut:].tobytes().decode())]


@pytest.mark.parametrize("K,iupac", [(31, False), (63, False), (30, False), (31, True)])
def test_canonical(K, iupac):
    sc, km, unsorted = kmers_of(canonical_genome(K, iupac), K, K)
    sba = sc.forward_sba
    order = oracle.canonical_sort(sba, unsorted, K)
    canon, is_rc = oracle.canonical_windows(sba, order, K)
    t = [bytes(r) for r in canon]
    km.sort(canonical=True)
    np.testing.assert_array_equal(km.kmer_sba_start_indices, order)
    rng = np.random.default_rng(K)
    raw = bytes(sba)
    picks = [raw[s:s + K] for s in order[rng.integers(0, len(order), 600)].tolist()]  # forward text, either strand
    queries = picks + [revcomp(x) for x in picks] + random_acgt(rng, 300, K)
    if K % 2 == 0:
        pal = raw[8000:8000 + K]
        assert revcomp(pal) == pal
        queries.append(pal)
    canon_q = [min(x, revcomp(x)) for x in queries]
    first, count = expect(t, canon_q)
    got_first, got_count = km.find(queries)
    np.testing.assert_array_equal(got_count, count)
    np.testing.assert_array_equal(got_first, first)
    np.testing.assert_array_equal(got_first[:600], got_first[600:1200])  # a query and its reverse complement
    np.testing.assert_array_equal(got_count[:600], got_count[600:1200])
    assert (count[:1200] > 0).all() and (count[1200:1500] == 0).all()
    if K % 2 == 0:
        assert count[-1] >= 2
    with pytest.raises(ValueError, match="canonical k-mers are grouped at kmer_len"):
        km.find("A" * (K - 1))
    with pytest.raises(_native.GkError) as e:
        km._engine.lookup(_native.pack_queries("A" * (K - 1)))
    assert e.value.code == _native.GK_E_ARG
    # strands of the hits: "-" where the canonical form is the reverse complement of the occurrence
    names = [n for n, _ in canonical_genome(K, iupac)]
    seg = sc._forward_sba_seg_starts.astype(np.int64)
    seen = set()
    for x in [raw[2000:2000 + K], raw[2100:2100 + K], revcomp(raw[2100:2100 + K]), raw[3000:3000 + K]] + picks[:40]:
        f, c = km.find(x)
        assert c > 0
        want = []
        for i in range(f, f + c):
            s = int(order[i])
            r = int(np.searchsorted(seg, s, side="right") - 1)
            want.append(("-" if is_rc[i] else "+", names[r], s - int(seg[r])))
        assert km.get_kmer_locations(x) == want
        seen |= {w[0] for w in want}
    assert seen == {"+", "-"}
    np.testing.assert_array_equal(km._engine.strand_range(0, len(order)), km.get_canonical_strands())


# ---------------------------------------------------------------------------------------------
# 10. the reference's tie order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_seed42_10kb_k5", "repeat_k31"])
def test_reference_tie_order(name):
    case, a = golden(name)
    sc = SequenceCollection(sequence_list=seq_list_of(case, a), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=case["min_kmer_len"], max_kmer_len=case["max_kmer_len"])
    km.sort(order="reference")
    np.testing.assert_array_equal(km.kmer_sba_start_indices, a["starts_default"])
    K = case["max_kmer_len"]
    t = golden_t(name, K)  # (the stable order: ties only permute the members of a group)
    present = sorted(set(t))
    check(km, t, present + mutate_last(present)[:500])


# ---------------------------------------------------------------------------------------------
# 11. the directory does not outlive the keys it indexes
# ---------------------------------------------------------------------------------------------
def test_directory_invalidation(monkeypatch):
    monkeypatch.setitem(_native.options, "GKM_LOOKUP_PATH", "keys")
    K = 21
    rng = np.random.default_rng(11)
    X = ACGT[rng.integers(0, 4, 5000)]
    Y = ACGT[rng.integers(0, 4, 8123)]
    seg = np.array([0], dtype=np.uint32)
    e = _native.Engine()
    tx = sorted(bytes(X[i:i + K]) for i in range(len(X) - K + 1))
    ty = sorted(bytes(Y[i:i + K]) for i in range(len(Y) - K + 1))
    queries = tx[::7] + ty[::7] + random_acgt(rng, 200, K)
    qa = _native.pack_queries(queries)
    e.set_sequence(X, seg)
    e.enumerate(K)
    with pytest.raises(_native.GkError) as err:  # enumerated, not sorted
        e.lookup(qa)
    assert err.value.code == _native.GK_E_STATE
    e.sort(K)
    first, count = e.lookup(qa)
    wf, wc = expect(tx, queries)
    np.testing.assert_array_equal(first, wf)
    np.testing.assert_array_equal(count, wc)
    e.set_sequence(Y, seg)
    with pytest.raises(_native.GkError) as err:
        e.lookup(qa)
    assert err.value.code == _native.GK_E_STATE
    e.enumerate(K)
    e.sort(K)
    first, count = e.lookup(qa)
    wf, wc = expect(ty, queries)
    np.testing.assert_array_equal(first, wf)
    np.testing.assert_array_equal(count, wc)
    # the same context re-sorted at another length: the directory is rebuilt for the new keys
    e.enumerate(12)
    e.sort(12)
    t12 = sorted(bytes(Y[i:i + 12]) for i in range(len(Y) - 12 + 1))
    q12 = t12[::5] + random_acgt(rng, 100, 12)
    first, count = e.lookup(_native.pack_queries(q12))
    wf, wc = expect(t12, q12)
    np.testing.assert_array_equal(first, wf)
    np.testing.assert_array_equal(count, wc)
    e.set_start_indices(np.arange(100, dtype=np.uint32), 12)
    with pytest.raises(_native.GkError) as err:
        e.lookup(_native.pack_queries(q12))
    assert err.value.code == _native.GK_E_STATE


# ---------------------------------------------------------------------------------------------
# 12. errors and trivia
# ---------------------------------------------------------------------------------------------
def test_errors_and_trivia():
    name = "repeat_k31"
    case, a = golden(name)
    K = case["max_kmer_len"]
    t = golden_t(name, K)
    sc = SequenceCollection(sequence_list=seq_list_of(case, a), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K, max_kmer_len=K)
    with pytest.raises(AssertionError, match="The kmers must be sorted when calling find"):
        km.find(t[0])
    km.sort()
    with pytest.raises(ValueError, match="more than max_kmer_len"):
        km.find("A" * (K + 1))
    present = t[len(t) // 2]
    for bad in (present[:-1].decode() + "a", present[:-1].decode() + "$", present[:-1].decode() + "X"):
        with pytest.raises(ValueError, match="outside the alphabet"):
            km.find([present.decode(), bad])
        check(km, t, [present])  # the context is still usable
    # the library's own check (Engine.lookup takes any bytes): refused on the host, nothing launched
    raw = _native.pack_queries([present, present]).copy()
    for byte in (ord("a"), ord("$"), ord("X"), 0):
        raw[1, 3] = byte
        with pytest.raises(_native.GkError, match=r"query 1 holds byte 0x%02x" % byte) as e:
            km._engine.lookup(raw)
        assert e.value.code == _native.GK_E_ALPHABET
        check(km, t, [present])
    # empty batches
    for empty in ([], np.zeros((0, K), dtype=np.uint8)):
        first, count = km.find(empty)
        assert first.dtype == np.uint64 and count.dtype == np.uint32 and first.shape == count.shape == (0,)
    # one str: scalars
    wf, wc = expect(t, [present])
    got = km.find(present.decode())
    assert got == (int(wf[0]), int(wc[0])) and all(type(v) is int for v in got)
    assert km.find(present) == got
    absent = mutate_last([present])[0]
    assert expect(t, [absent])[1][0] == 0
    assert km.count(present) == int(wc[0]) and km.count(absent) == 0
    assert present in km and present.decode() in km and absent not in km


@pytest.mark.parametrize("name", ["repeat_k31", "seq2_min3_max3", "iupac_k31"])
def test_kmer_locations(name):
    case, a = golden(name)
    K = case["max_kmer_len"]
    t = golden_t(name, K)
    km = sorted_kmers(name)
    seg = a["seg_starts"].astype(np.int64)
    starts = a["starts_stable"].astype(np.int64)
    assert len(seg) > 1
    rng = np.random.default_rng(3)
    multi = [x for x in sorted(set(t)) if bisect_right(t, x) - bisect_left(t, x) > 1]
    picks = multi[:20] + [t[i] for i in rng.integers(0, len(t), 20)]
    if name == "repeat_k31":
        assert len(multi) >= 20
    for one_based in (False, True):
        for x in picks:
            f, l = bisect_left(t, x), bisect_right(t, x)
            rec = np.searchsorted(seg, starts[f:l], side="right") - 1
            want = [("+", case["record_names"][r], int(s - seg[r]) + int(one_based))
                    for s, r in zip(starts[f:l].tolist(), rec.tolist())]
            assert km.get_kmer_locations(x, one_based_seq_index=one_based) == want
    absent = next(x for x in mutate_last(sorted(set(t))) if bisect_right(t, x) == bisect_left(t, x))
    assert km.get_kmer_locations(absent) == []
