"""K-mer search with mismatches on the device: gk_lookup_mismatch through Kmers.count_near / find_near /
get_near_locations and _native.Engine.mismatch_counts / mismatch_hits, on both paths (bytes, keys).

The expected values never come from the code under test.  ``brute`` works on the host sba and a start
order that is itself computed on the host (the golden ``starts_stable``, the oracle's enumeration, a
host sort): for every start it takes the q bytes there, drops the start if they hold '$' or run past
the end, and counts ``(window != query).sum()`` against the query and -- both strands -- against its
reverse complement, whose complement table is spelt out below.  Counts by distance and the hit list in
ascending (query, position in the order, strand) follow from that.

Every parametrised case asserts on that brute-force expectation that the case is not trivial: at least
one hit at every distance 0..max_mismatches (where max_mismatches <= 3), and at least one query without
any hit where one can exist -- max_mismatches < q and q >= 16.  (A shorter query, or one allowed q
mismatches, is within reach of some k-mer of any genome that holds all four bases: 1 - P(no hit) is 1
to many digits at q <= 2 for a few hundred k-mers.)  Queries are windows of the genome with 0, 1, 2, ...
planted substitutions, which gives the hits by construction, plus random strings, which at q >= 16
and d <= 3 lie within reach of one of ~10^4 k-mers with probability below 10^-3 each.  The manifest's
small cases (37-base genomes with q <= 9, the 5-mers of a 10 kb genome) run sorted and unsorted too,
asserting a hit at every planted distance; no string of their length is without a hit at d = min(3, q).
"""

from functools import lru_cache

import ctypes

import numpy as np
import pytest

from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection
from oracle import oracle

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in load_manifest()}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DOLLAR = ord("$")
R_TILE = 4 * 256  # k-mers per block and step of the scan (kMismatchR x 256 threads)

# the reference's IUPAC complement (sequence_collection.py:402-433), spelt out
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B",
              "D": "H", "H": "D", "S": "S", "W": "W", "N": "N"}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in COMPLEMENT.items():
    COMP[ord(_a)] = ord(_b)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# host expectations
# ---------------------------------------------------------------------------------------------
def revcomp(x: bytes) -> bytes:
    return bytes(COMP[np.frombuffer(x, dtype=np.uint8)][::-1])


def windows(sba, order, q):
    """(the q bytes at every start of the order, whether the start takes part)"""
    sba = np.asarray(sba, dtype=np.uint8)
    padded = np.concatenate([sba, np.full(q, DOLLAR, dtype=np.uint8)])  # past the end reads as '$'
    win = padded[np.asarray(order, dtype=np.int64)[:, None] + np.arange(q)]
    return win, ~(win == DOLLAR).any(axis=1)


def brute(sba, order, queries, maxd, both):
    """counts uint64[m, maxd + 1] and the hit arrays (query, kmer_num, mismatches, strand)"""
    q = len(queries[0])
    win, ok = windows(sba, order, q)
    counts = np.zeros((len(queries), maxd + 1), dtype=np.uint64)
    hq, hn, hm, hs = [], [], [], []
    for j, x in enumerate(queries):
        forms = [np.frombuffer(x, dtype=np.uint8)]
        if both:
            forms.append(COMP[forms[0]][::-1])
        pos, dist, strand = [], [], []
        for s, f in enumerate(forms):
            d = (win != f).sum(axis=1)
            sel = np.flatnonzero(ok & (d <= maxd))
            pos.append(sel)
            dist.append(d[sel])
            strand.append(np.full(len(sel), s))
        pos, dist, strand = np.concatenate(pos), np.concatenate(dist), np.concatenate(strand)
        by = np.lexsort((strand, pos))
        counts[j] = np.bincount(dist, minlength=maxd + 1)[:maxd + 1]
        hq.append(np.full(len(by), j))
        hn.append(pos[by])
        hm.append(dist[by])
        hs.append(strand[by])
    hits = (np.concatenate(hq).astype(np.uint32), np.concatenate(hn).astype(np.uint64),
            np.concatenate(hm).astype(np.uint8), np.concatenate(hs).astype(np.uint8))
    return counts, hits


NEXT = {65: 67, 67: 71, 71: 84, 84: 65}  # A -> C -> G -> T -> A; any other letter -> A


def make_queries(rng, sba, order, q, maxd, n_windows=40, n_random=10):
    """windows of the genome with i % (min(maxd, 3) + 1) planted substitutions, then random strings"""
    win, ok = windows(sba, order, q)
    full = np.flatnonzero(ok)
    assert len(full) > 0
    out = []
    for i in range(n_windows):
        w = win[full[rng.integers(0, len(full))]].copy()
        for p in rng.choice(q, size=min(i % (min(maxd, 3) + 1), q), replace=False).tolist():
            w[p] = NEXT.get(int(w[p]), 65)
        out.append(bytes(w))
    return out + [bytes(r) for r in ACGT[rng.integers(0, 4, (n_random, q))]]


def is_acgt(x) -> bool:
    return bool(np.isin(np.frombuffer(bytes(x), dtype=np.uint8), ACGT).all())


def check(monkeypatch, km, sba, order, queries, maxd, both, keys, nontrivial=True):
    """count_near and find_near equal the brute force on auto, bytes and -- where `keys` says the
    key path applies -- keys; a forced key path where it does not apply is refused"""
    q = len(queries[0])
    want_counts, want_hits = brute(sba, order, queries, maxd, both)
    if nontrivial and maxd <= 3:
        assert (want_counts.sum(axis=0) > 0).all(), "a distance without any hit"
    if nontrivial is True and maxd < q and q >= 16:  # ("hits": a genome too small for a query without a hit)
        assert (want_counts.sum(axis=1) == 0).any(), "no query without a hit"
    for path in ("auto", "bytes", "keys"):
        if path != "auto":
            monkeypatch.setitem(_native.options, "GKM_MISMATCH_PATH", path)
        if path == "keys" and not keys:
            with pytest.raises(_native.GkError) as e:
                km.count_near(queries, maxd, both)
            assert e.value.code == _native.GK_E_UNSUPPORTED
            continue
        got_counts = km.count_near(queries, maxd, both)
        assert got_counts.dtype == np.uint64 and got_counts.shape == want_counts.shape
        np.testing.assert_array_equal(got_counts, want_counts)
        got = km.find_near(queries, maxd, both)
        assert [g.dtype for g in got] == [np.uint32, np.uint64, np.uint8, np.uint8]
        for g, w in zip(got, want_hits):
            np.testing.assert_array_equal(g, w)
    monkeypatch.delitem(_native.options, "GKM_MISMATCH_PATH", raising=False)
    return want_counts, want_hits


def host_sorted(sba, starts, K):
    """The stable order (k-mer cut at K, then start) of the given starts, sorted on the host."""
    raw = bytes(np.asarray(sba, dtype=np.uint8))
    pairs = sorted((raw[s:s + K].split(b"$")[0] if K else raw[s:].split(b"$")[0], s) for s in starts.tolist())
    return np.array([s for _, s in pairs], dtype=np.uint32)


def kmers_of(seqs, kmin, kmax):
    """(sc, km, the enumeration order computed by the oracle)"""
    sc = SequenceCollection(sequence_list=seqs, strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=kmin, max_kmer_len=kmax)
    return sc, km, oracle.enumerate_starts(sc.forward_sba, sc._forward_sba_seg_starts, kmin)


# ---------------------------------------------------------------------------------------------
# 1. golden cases
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def golden(name):
    case = CASES[name]
    a = load_case(name)
    for v in a.values():
        v.setflags(write=False)
    return case, a


def golden_qlen(case):
    return 20 if case["max_kmer_len"] is None else min(case["max_kmer_len"], 32)


# The manifest's cases whose genome can hold the expectations above at max_mismatches = 3: q >= 20.
# (The seq2 cases, 37 bases with q <= 9, and the 5-mers of c1_seed42_10kb_k5 leave no string without a
# hit within 3; they run in test_tiny_golden_cases, which asserts a hit at every distance only.)
GOLDEN = [c["name"] for c in CASES.values() if len(load_case(c["name"])["sba"]) > 100 and golden_qlen(c) >= 20]
TINY = [c["name"] for c in CASES.values() if c["name"] not in GOLDEN]


def golden_keys(case, a):
    """The key path serves the sorted case: ACGT-only sba, one fixed length of at most 32 bases."""
    return (case["min_kmer_len"] == case["max_kmer_len"] and case["max_kmer_len"] is not None
            and case["max_kmer_len"] <= 32 and bool(np.isin(a["sba"], np.frombuffer(b"ACGT$", dtype=np.uint8)).all()))


def golden_kmers(name, do_sort):
    case, a = golden(name)
    sc = SequenceCollection(sequence_list=seq_list_of(case, a), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=case["min_kmer_len"], max_kmer_len=case["max_kmer_len"])
    if do_sort:
        km.sort()
        return km, a["starts_stable"]
    return km, oracle.enumerate_starts(a["sba"], a["seg_starts"], case["min_kmer_len"])


def test_golden_selection():
    assert set(GOLDEN) == {"rand10k_k31", "iupac_k31", "repeat_k31", "repeat_k40", "repeat_min10_max40",
                           "repeat_suffix_min4", "iupac_min6_max25", "iupac_suffix_min2"}


@pytest.mark.parametrize("do_sort", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("both", [False, True], ids=["forward", "both"])
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_cases(name, both, do_sort, monkeypatch):
    case, a = golden(name)
    q = golden_qlen(case)
    km, order = golden_kmers(name, do_sort)
    rng = np.random.default_rng(len(name) + q)
    queries = make_queries(rng, a["sba"], order, q, 3)
    keys = do_sort and golden_keys(case, a) and all(is_acgt(x) for x in queries)
    check(monkeypatch, km, a["sba"], order, queries, 3, both, keys)


@pytest.mark.parametrize("do_sort", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("name", TINY)
def test_tiny_golden_cases(name, do_sort, monkeypatch):
    """every other case of the manifest (37-base genomes, 5-mers) at min(3, q) mismatches, forward and
    both strands: a hit at every planted distance; no string of that length is without a hit there"""
    case, a = golden(name)
    q = min(case["max_kmer_len"] or 6, 32)
    maxd = min(3, q)
    km, order = golden_kmers(name, do_sort)
    rng = np.random.default_rng(q)
    queries = make_queries(rng, a["sba"], order, q, maxd, n_windows=8, n_random=4)
    for both in (False, True):
        check(monkeypatch, km, a["sba"], order, queries, maxd, both, do_sort and golden_keys(case, a),
              nontrivial="hits")


# ---------------------------------------------------------------------------------------------
# 2. kernel-shape edges on a synthetic A/C/G/T genome
# ---------------------------------------------------------------------------------------------
def edge_genome(n, K):
    """one contig with exactly n K-mers; runs of T and of A (40 each) where there is room"""
    rng = np.random.default_rng(1000 * K + n)
    s = ACGT[rng.integers(0, 4, n + K - 1)].copy()
    if len(s) >= 200:
        s[10:50] = ord("T")
        s[100:140] = ord("A")
    return s


@pytest.mark.parametrize("mode", ["K=q", "K=32"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, R_TILE - 1, R_TILE + 1, 3000])
def test_kernel_shape_edges(n, mode, monkeypatch):
    for q in (1, 2, 16, 17, 31, 32):
        K = q if mode == "K=q" else 32
        if mode == "K=32" and q == 32:
            continue  # (K=q's case)
        s = edge_genome(n, K)
        sc, km, unsorted = kmers_of([("c0", s.tobytes().decode())], K, K)
        assert len(unsorted) == n
        sba = sc.forward_sba
        order = host_sorted(sba, unsorted, K)
        km.sort()
        rng = np.random.default_rng(n + q)
        for maxd in (0, 1, q):
            queries = make_queries(rng, sba, order, q, maxd, n_windows=12, n_random=4) + [b"T" * q, b"A" * q]
            # (a single k-mer is not sorted, so the context holds no keys)
            counts, _ = check(monkeypatch, km, sba, order, queries, maxd, maxd == 1, n >= 2)
            if len(s) >= 200:  # the all-T and all-A words are present: key all ones and key 0
                assert counts[-2, 0] >= 40 - max(q, K) + 1 and counts[-1, 0] >= 40 - max(q, K) + 1
            if maxd == q:  # every k-mer is within q of every query, on every strand compared
                assert (counts.sum(axis=1) == n * (2 if maxd == 1 else 1)).all()


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both"])
@pytest.mark.parametrize("chunk,m", [(None, 1), ("20", 21), ("20", 50), ("1", 3)])
def test_chunked_launches(chunk, m, both, monkeypatch):
    """m = 1; m = chunk + 1 (two launches); three launches, the last one partial; one query each"""
    if chunk:
        monkeypatch.setitem(_native.options, "GKM_MISMATCH_CHUNK", chunk)
    K = 20
    s = edge_genome(2500, K)
    sc, km, unsorted = kmers_of([("c0", s.tobytes().decode())], K, K)
    order = host_sorted(sc.forward_sba, unsorted, K)
    km.sort()
    rng = np.random.default_rng(m)
    queries = make_queries(rng, sc.forward_sba, order, K, 3, n_windows=m - min(8, m - 1), n_random=min(8, m - 1))
    assert len(queries) == m
    # the knob is obeyed: the launches of one call, and the pairs they cover, from the context's profile
    eng = km._engine
    eng.profile_enable(True)
    km.count_near(queries, 3, both)
    report = eng.profile_report()
    eng.profile_enable(False)
    launches = -(-m // int(chunk)) if chunk else 1
    assert launches == {(None, 1): 1, ("20", 21): 2, ("20", 50): 3, ("1", 3): 3}[(chunk, m)]
    assert report["mismatch_keys"]["count"] == launches and report["mismatch_keys"]["units"] == len(order) * m
    if m >= 21:
        check(monkeypatch, km, sc.forward_sba, order, queries, 3, both, True)
    else:  # too few queries for a hit at every distance
        counts, _ = check(monkeypatch, km, sc.forward_sba, order, queries, 3, both, True, nontrivial=False)
        if m == 3:
            assert counts.sum() > 0 and (counts.sum(axis=1) == 0).any()


# ---------------------------------------------------------------------------------------------
# 3. short contigs and contig ends
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmin,kmax", [(1, 20), (4, None), (20, 20)])
def test_short_contigs_and_contig_ends(kmin, kmax, monkeypatch):
    q = 20
    rng = np.random.default_rng(77)
    # contigs shorter than q among them (none shorter than min_kmer_len: the reference's enumeration has no such contig)
    lens = [max(L, kmin) for L in (300, 250, 7, 19, 20, 21, 1, 12)]
    seqs = [(f"c{i}", bytes(ACGT[rng.integers(0, 4, L)]).decode()) for i, L in enumerate(lens)]
    sc, km, unsorted = kmers_of(seqs, kmin, kmax)
    sba = sc.forward_sba
    _, ok = windows(sba, unsorted, q)
    if kmin < q:
        assert (~ok).sum() >= 50, "starts whose k-mer meets '$' before q bytes must be present"
    else:
        assert ok.all()
    raw = bytes(sba)
    for do_sort in (False, True):
        order = unsorted
        if do_sort:
            order = host_sorted(sba, unsorted, kmax)
            km.sort()
        queries = make_queries(rng, sba, order, q, 3)
        # strings that exist only across a '$' (the '$' replaced by each base): never a hit at d = 0
        at = raw.index(b"$")
        queries += [raw[at - 10:at] + b + raw[at + 1:at + 10] for b in (b"A", b"C", b"G", b"T")]
        keys = do_sort and kmin == kmax
        counts, hits = check(monkeypatch, km, sba, order, queries, 3, True, keys)
        short = np.flatnonzero(~windows(sba, order, q)[1])
        got = km.find_near(queries, 3, True)
        assert not np.isin(got[1], short).any()


# ---------------------------------------------------------------------------------------------
# 4. mixed alphabet
# ---------------------------------------------------------------------------------------------
def mixed_genome():
    rng = np.random.default_rng(12)
    seqs = []
    for i, L in enumerate((6000, 2500)):
        s = ACGT[rng.integers(0, 4, L)].copy()
        for _ in range(4):
            at = int(rng.integers(0, L - 200))
            s[at:at + int(rng.integers(25, 120))] = ord("N")
        s[1000:1040:3] = ord("R")
        s[1500:1540:4] = ord("Y")
        s[2000:2030:5] = np.frombuffer(b"KMBDHV", dtype=np.uint8)
        s[2200:2230:7] = np.frombuffer(b"SWSWS", dtype=np.uint8)
        seqs.append((f"c{i}", s.tobytes().decode()))
    return seqs


@pytest.mark.parametrize("both", [False, True], ids=["forward", "both"])
@pytest.mark.parametrize("K,q", [(31, 31), (31, 20), (40, 32)])
def test_mixed_alphabet(K, q, both, monkeypatch):
    sc, km, unsorted = kmers_of(mixed_genome(), K, K)
    sba = sc.forward_sba
    order = host_sorted(sba, unsorted, K)
    km.sort()
    rng = np.random.default_rng(K + q)
    queries = make_queries(rng, sba, order, q, 3)
    raw = bytes(sba)
    n_edges = np.flatnonzero((sba[1:] == ord("N")) != (sba[:-1] == ord("N"))).tolist()
    straddle = [raw[p - j:p - j + q] for p in n_edges for j in (1, q // 2) if p - j >= 0
                and len(raw[p - j:p - j + q]) == q and b"$" not in raw[p - j:p - j + q]]
    iupac = [raw[1000:1000 + q], raw[1990:1990 + q], raw[2195:2195 + q]]
    queries += straddle[:10] + iupac + [b"N" * q, b"N" * (q - 1) + b"A", b"A" + b"N" * (q - 1)]
    assert len(straddle) >= 4 and all(not is_acgt(x) for x in iupac)
    counts, _ = check(monkeypatch, km, sba, order, queries, 3, both, False)  # (a forced key path is refused)
    k = len(queries) - 3
    assert counts[k, 0] > 0  # N x q is present: 'N' against 'N' is a match
    assert counts[k + 1, 1] > 0 and counts[k + 2, 1] > 0  # ... and one 'A' against an 'N' is one mismatch
    assert (counts[-6:-3, 0] > 0).all()
    # an all-A/C/G/T batch: still the byte path, because the index holds 4-bit keys -- a forced key
    # path is refused for the context, not for the queries
    plain = [x for x in queries if is_acgt(x)]
    assert len(plain) >= 20
    check(monkeypatch, km, sba, order, plain, 3, both, False)
    monkeypatch.setitem(_native.options, "GKM_MISMATCH_PATH", "keys")
    with pytest.raises(_native.GkError, match="holds no final one-word 2-bit forward keys") as e:
        km.count_near(plain, 3, both)
    assert e.value.code == _native.GK_E_UNSUPPORTED


def test_iupac_queries_on_an_acgt_index(monkeypatch):
    """final 2-bit keys, but a query with a letter outside A/C/G/T: the byte path, the key path refused"""
    K = 24
    s = edge_genome(3000, K)
    sc, km, unsorted = kmers_of([("c0", s.tobytes().decode())], K, K)
    order = host_sorted(sc.forward_sba, unsorted, K)
    km.sort()
    rng = np.random.default_rng(2)
    queries = make_queries(rng, sc.forward_sba, order, K, 3)
    check(monkeypatch, km, sc.forward_sba, order, queries, 3, True, True)
    with_n = [x[:5] + b"N" + x[6:] for x in queries[:12]] + queries[12:]
    counts, _ = check(monkeypatch, km, sc.forward_sba, order, with_n, 3, True, False)
    assert (counts[:, 0] == 0)[:12].all()


# ---------------------------------------------------------------------------------------------
# 5. other orders: kmer_num refers to the order actually held
# ---------------------------------------------------------------------------------------------
def order_genome(K):
    rng = np.random.default_rng(900 + K)
    s = ACGT[rng.integers(0, 4, 6000)].copy()
    s[4000:4200] = COMP[s[1000:1200]][::-1]  # both strands of one stretch
    s[5000:5100] = s[2000:2100]
    cut = 3500
    return [("c0", s[:cut].tobytes().decode()), ("c1", s[cut:].tobytes().decode())]


@pytest.mark.parametrize("kind", ["canonical", "subset", "permutation", "reference"])
def test_other_orders(kind, monkeypatch):
    K = 22
    sc, km, unsorted = kmers_of(order_genome(K), K, K)
    sba = sc.forward_sba
    rng = np.random.default_rng(len(kind))
    keys = False
    if kind == "canonical":
        order = oracle.canonical_sort(sba, unsorted, K)
        km.sort(canonical=True)
    elif kind == "subset":
        order = np.sort(rng.choice(unsorted, size=len(unsorted) // 3, replace=False)).astype(np.uint32)
        km.kmer_sba_start_indices = order.copy()
    elif kind == "permutation":
        order = rng.permutation(unsorted).astype(np.uint32)
        km.kmer_sba_start_indices = order.copy()
    else:
        km.sort(order="reference")
        order = km.kmer_sba_start_indices.copy()  # ties in numba's order: checked to be a sorted order
        cut = [bytes(sba[s:s + K]) for s in order.tolist()]
        assert cut == sorted(cut) and sorted(order.tolist()) == sorted(unsorted.tolist())
        keys = None
    np.testing.assert_array_equal(km.kmer_sba_start_indices, order)
    queries = make_queries(rng, sba, order, K, 3)
    if keys is None:  # (whether the host-ordered sort keeps usable keys is the library's business: auto and bytes)
        want_counts, want_hits = brute(sba, order, queries, 3, True)
        for path in ("auto", "bytes"):
            if path != "auto":
                monkeypatch.setitem(_native.options, "GKM_MISMATCH_PATH", path)
            np.testing.assert_array_equal(km.count_near(queries, 3, True), want_counts)
            for g, w in zip(km.find_near(queries, 3, True), want_hits):
                np.testing.assert_array_equal(g, w)
        assert (want_counts.sum(axis=0) > 0).all() and (want_counts.sum(axis=1) == 0).any()
    else:
        check(monkeypatch, km, sba, order, queries, 3, True, keys)
    # q shorter and longer than the sort length: the scan is not tied to it
    for q in (9, 30):
        qs = make_queries(rng, sba, order, q, 2, n_windows=9, n_random=3)
        want_counts, want_hits = brute(sba, order, qs, 2, False)
        np.testing.assert_array_equal(km.count_near(qs, 2), want_counts)
        for g, w in zip(km.find_near(qs, 2), want_hits):
            np.testing.assert_array_equal(g, w)


# ---------------------------------------------------------------------------------------------
# 6. both strands
# ---------------------------------------------------------------------------------------------
def test_both_strands(monkeypatch):
    K = 20
    rng = np.random.default_rng(20)
    s = ACGT[rng.integers(0, 4, 5000)].copy()
    half = ACGT[rng.integers(0, 4, K // 2)]
    pal = np.concatenate([half, COMP[half][::-1]])
    assert revcomp(bytes(pal)) == bytes(pal)
    s[700:700 + K] = pal
    s[2100:2100 + K] = pal
    near = pal.copy()
    near[3] = NEXT[int(near[3])]  # one substitution away on the forward strand (and on the reverse one)
    s[3300:3300 + K] = near
    s[4000:4200] = COMP[s[1000:1200]][::-1]
    sc, km, unsorted = kmers_of([("c0", s.tobytes().decode())], K, K)
    sba = sc.forward_sba
    order = host_sorted(sba, unsorted, K)
    km.sort()
    queries = [bytes(pal)] + make_queries(rng, sba, order, K, 3)
    counts, hits = check(monkeypatch, km, sba, order, queries, 3, True, True)
    # the reverse palindrome: each site twice, strand 0 before strand 1
    hq, hn, hm, hs = km.find_near(queries, 3, True)
    mine = hq == 0
    assert counts[0, 0] == 4 and counts[0, 1] == 2
    exact = mine & (hm == 0)
    np.testing.assert_array_equal(hs[exact], [0, 1, 0, 1])
    assert hn[exact][0] == hn[exact][1] and hn[exact][2] == hn[exact][3] and hn[exact][0] != hn[exact][2]
    assert set(order[hn[exact]].tolist()) == {700, 2100}
    # a query and its reverse complement: the same counts, the strands swapped
    rc_queries = [revcomp(x) for x in queries]
    np.testing.assert_array_equal(km.count_near(rc_queries, 3, True), counts)
    fwd = km.count_near(queries, 3, False)
    rev = km.count_near(rc_queries, 3, False)
    np.testing.assert_array_equal(fwd + rev, counts)
    assert rev.sum() > 0  # (the planted reverse-strand stretch)


# ---------------------------------------------------------------------------------------------
# 7. cross-check with the exact lookup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "bytes", "keys"])
def test_distance_zero_is_find(path, monkeypatch):
    if path != "auto":
        monkeypatch.setitem(_native.options, "GKM_MISMATCH_PATH", path)
    name = "repeat_k31"
    case, a = golden(name)
    km, order = golden_kmers(name, True)
    rng = np.random.default_rng(31)
    queries = make_queries(rng, a["sba"], order, 31, 0, n_windows=60, n_random=20)
    first, count = km.find(queries)
    counts = km.count_near(queries, 0)
    np.testing.assert_array_equal(counts[:, 0], count)
    assert (count > 1).any() and (count == 0).any()
    hq, hn, hm, hs = km.find_near(queries, 0)
    want_q = np.repeat(np.arange(len(queries)), count)
    want_n = np.concatenate([np.arange(f, f + c) for f, c in zip(first.tolist(), count.tolist())])
    np.testing.assert_array_equal(hq, want_q)
    np.testing.assert_array_equal(hn, want_n)
    assert not hm.any() and not hs.any()


# ---------------------------------------------------------------------------------------------
# 8. API behaviour
# ---------------------------------------------------------------------------------------------
def test_api_behaviour():
    name = "repeat_k31"
    case, a = golden(name)
    km, order = golden_kmers(name, False)  # no sort needed
    sba = a["sba"]
    rng = np.random.default_rng(8)
    queries = make_queries(rng, sba, order, 31, 2)
    want_counts, want_hits = brute(sba, order, queries, 2, True)
    total = int(want_counts.sum())
    assert total >= 40
    # one str / bytes: a 1-D counts row
    one = km.count_near(queries[1].decode(), 2, True)
    assert one.shape == (3,) and one.dtype == np.uint64
    np.testing.assert_array_equal(one, want_counts[1])
    np.testing.assert_array_equal(km.count_near(queries[1], 2, True), want_counts[1])
    # max_hits
    with pytest.raises(ValueError, match=rf"\b{total}\b"):
        km.find_near(queries, 2, True, max_hits=total - 1)
    for g, w in zip(km.find_near(queries, 2, True, max_hits=total), want_hits):
        np.testing.assert_array_equal(g, w)
    # the C ABI: a capacity one short of *n_hits is refused with the number; counts and *n_hits stand
    eng, lib = km._engine, km._engine.lib
    q = _native.pack_queries(queries)
    m, qlen = q.shape
    counts = np.zeros((m, 3), dtype=np.uint64)
    hq, hn = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint64)
    hm, hs = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
    n_hits = ctypes.c_uint64(0)

    def call(cap, d=2, hit_q=hq, hit_s=hs, flags=_native.MISMATCH_BOTH_STRANDS, qq=q, length=qlen, rows=m):
        p = _native._ptr
        return lib.gk_lookup_mismatch(eng.ctx, p(qq, ctypes.c_uint8), rows, length, d, flags,
                                      p(counts, ctypes.c_uint64), None if hit_q is None else p(hit_q, ctypes.c_uint32),
                                      p(hn, ctypes.c_uint64), p(hm, ctypes.c_uint8),
                                      None if hit_s is None else p(hit_s, ctypes.c_uint8), cap, ctypes.byref(n_hits))

    assert call(total - 1) == _native.GK_E_ARG
    assert str(total) in lib.gk_last_error(eng.ctx).decode() and n_hits.value == total
    np.testing.assert_array_equal(counts, want_counts)
    assert call(total) == _native.GK_OK and n_hits.value == total
    for g, w in zip((hq, hn, hm, hs), want_hits):
        np.testing.assert_array_equal(g, w)
    assert call(0, hit_q=None) == _native.GK_OK and n_hits.value == total  # counts only
    assert call(total, hit_s=None) == _native.GK_E_ARG  # a hit array missing
    assert call(total, flags=2) == _native.GK_E_ARG and call(total, flags=3) == _native.GK_E_ARG
    assert call(total, d=32) == _native.GK_E_ARG  # max_mismatches > qlen
    wide = np.full((2, 33), ord("A"), dtype=np.uint8)
    assert call(total, qq=wide, length=33, rows=2) == _native.GK_E_ARG
    assert call(total, length=0) == _native.GK_E_ARG
    n_hits.value = 99
    before = counts.copy()
    assert call(total, rows=0) == _native.GK_OK and n_hits.value == 0  # an empty batch touches nothing else
    np.testing.assert_array_equal(counts, before)
    bad = q.copy()
    bad[3, 4] = ord("x")
    assert call(total, qq=bad) == _native.GK_E_ALPHABET
    assert "query 3 holds byte 0x78" in lib.gk_last_error(eng.ctx).decode()
    # the Python surface
    with pytest.raises(ValueError, match="max_mismatches"):
        km.count_near(queries, 32)
    with pytest.raises(ValueError, match="max_mismatches"):
        km.find_near(queries, -1)
    with pytest.raises(ValueError, match="more than 32"):
        km.count_near("A" * 33, 1)
    with pytest.raises(ValueError, match="outside the alphabet"):
        km.count_near("ACGTx", 1)
    for empty in ([], np.zeros((0, 31), dtype=np.uint8)):
        c = km.count_near(empty, 2)
        assert c.shape == (0, 3) and c.dtype == np.uint64
        got = km.find_near(empty, 2)
        assert [len(g) for g in got] == [0, 0, 0, 0]
        assert [g.dtype for g in got] == [np.uint32, np.uint64, np.uint8, np.uint8]
    # still usable after every refusal
    np.testing.assert_array_equal(km.count_near(queries, 2, True), want_counts)


def test_more_hits_than_the_first_record_buffer(monkeypatch):
    """more than 2^20 hits: the hits call scans a second time into a buffer of the size found"""
    K = 8
    s = edge_genome(3000, K)
    sc, km, unsorted = kmers_of([("c0", s.tobytes().decode())], K, K)
    order = host_sorted(sc.forward_sba, unsorted, K)
    km.sort()
    rng = np.random.default_rng(5)
    queries = make_queries(rng, sc.forward_sba, order, K, K, n_windows=300, n_random=100)
    counts, hits = check(monkeypatch, km, sc.forward_sba, order, queries, K, False, True, nontrivial=False)
    assert len(hits[0]) == 400 * 3000 > 1 << 20
    # and a small search on the same context afterwards
    check(monkeypatch, km, sc.forward_sba, order, queries[:50], 1, True, True, nontrivial=False)


def test_state_errors():
    e = _native.Engine()
    q = _native.pack_queries(["ACGTACGT"])
    with pytest.raises(_native.GkError) as err:
        e.mismatch_counts(q, 1)
    assert err.value.code == _native.GK_E_STATE
    s = ACGT[np.random.default_rng(1).integers(0, 4, 500)]
    e.set_sequence(s, np.array([0], dtype=np.uint32))
    with pytest.raises(_native.GkError) as err:
        e.mismatch_counts(q, 1)
    assert err.value.code == _native.GK_E_STATE
    e.enumerate(8)  # enumerated, never sorted: enough
    want_counts, want_hits = brute(s, np.arange(500 - 8 + 1), [bytes(s[40:48]), b"ACGTACGT"], 1, False)
    counts, *hits = e.mismatch_hits(_native.pack_queries([bytes(s[40:48]), b"ACGTACGT"]), 1)
    np.testing.assert_array_equal(counts, want_counts)
    for g, w in zip(hits, want_hits):
        np.testing.assert_array_equal(g, w)
    assert want_counts[0, 0] >= 1


@pytest.mark.parametrize("name", ["repeat_k31", "iupac_k31"])
def test_near_locations(name):
    case, a = golden(name)
    km, order = golden_kmers(name, True)
    sba = a["sba"]
    seg = a["seg_starts"].astype(np.int64)
    assert len(seg) > 1
    rng = np.random.default_rng(4)
    queries = make_queries(rng, sba, order, 31, 2, n_windows=12, n_random=2)
    seen = set()
    for one_based in (False, True):
        for x in queries:
            _, (hq, hn, hm, hs) = brute(sba, order, [x], 2, True)
            starts = np.asarray(order, dtype=np.int64)[hn.astype(np.int64)]
            rec = np.searchsorted(seg, starts, side="right") - 1
            want = [("-" if st else "+", case["record_names"][r], int(s - seg[r]) + int(one_based), int(mm))
                    for st, r, s, mm in zip(hs.tolist(), rec.tolist(), starts.tolist(), hm.tolist())]
            assert km.get_near_locations(x, 2, both_strands=True, one_based_seq_index=one_based) == want
            seen |= {(w[0], w[3]) for w in want}
    assert {("+", 0), ("+", 1), ("+", 2)} <= seen
    assert km.get_near_locations(queries[-1], 2) == []
    with pytest.raises(ValueError, match="one k-mer"):
        km.get_near_locations([queries[0]], 2)
