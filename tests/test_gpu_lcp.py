"""The LCP array of the sorted order on the device: gk_lcp, gk_lcp_spectrum and gk_position_track
through Kmers.lcp / kmer_spectrum / min_unique_lengths / multiplicity_track and _native.Engine, on both
paths (keys, bytes).

Every expectation comes from tests/lcpref.py (numpy on the host sba and the sorted starts: the two
windows walked byte by byte with the '$' rules) and never from the code under test.  Every parametrised
case first asserts on that reference alone that it is not trivial: lcp takes the value 0, the value cap
and at least three values between them, and unique[cap] < n.  TILE, THREADS and LDS_BINS mirror
gkm_lcp_host.h (tests/test_lcp_host.py reads them from the header), SCAN_TILE gkm_internal.h's kScanTile,
GRID_CAP the kernels' grid cap.
"""

from collections import Counter

import numpy as np
import pytest

import lcpref
from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection

pytestmark = pytest.mark.gpu

THREADS, TILE, LDS_BINS, SCAN_TILE, GRID_CAP = 256, 1024, 1024, 4096, 2048
CASES = {c["name"]: c for c in load_manifest()}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NEXT = {65: 67, 67: 71, 71: 84, 84: 65}  # a substitution: A->C->G->T->A


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# genomes
# ---------------------------------------------------------------------------------------------
def rand_seq(seed, n, letters=b"ACGT") -> str:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


SWEEP_LEN = 102


def sweep_seqs(seed, copies=SWEEP_LEN, tails=None):
    """Copies of one random 102-mer as separate contigs, copy t carrying one substitution at offset t:
    the k-mers at offset 0 of copies t < k differ from every other copy's exactly at t, so every LCP
    value 0..k occurs between sorted neighbours (k <= 100); ``tails``: one letter appended per contig."""
    base = ACGT[np.random.default_rng(seed).integers(0, 4, SWEEP_LEN)].copy()
    seqs = []
    for t in range(copies):
        c = base.copy()
        c[t] = NEXT[int(c[t])]
        seqs.append((f"s{t}", c.tobytes().decode() + (tails[t % len(tails)] if tails else "")))
    return seqs


def edge_seqs(seed, copies, k, n_target):
    """The sweep behind a random contig whose length makes the genome hold exactly n_target k-mers."""
    prefix = n_target - copies * (SWEEP_LEN - k + 1) + k - 1
    assert prefix >= k
    return [("p", rand_seq(seed, prefix))] + sweep_seqs(seed + 1000, copies)


def golden_seqs(name):
    return seq_list_of(CASES[name], load_case(name))


def is_acgt(seqs) -> bool:
    return all(set(s) <= set("ACGT") for _, s in seqs)


def keys_eligible(seqs, kmin, kmax) -> bool:
    """The key path serves the sort: direct keys of at most 256 bits without a length field -- one
    fixed length on A/C/G/T data (2 bits), any bounds on a mixed alphabet (4 bits, '$' is a code)."""
    if kmax is None:
        return False
    return (kmin == kmax and 2 * kmax <= 256) if is_acgt(seqs) else 4 * kmax <= 256


def sorted_kmers(seqs, kmin, kmax, canonical=False):
    sc = SequenceCollection(sequence_list=seqs, strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=kmin, max_kmer_len=kmax)
    km.sort(canonical=canonical)
    return km


def host_view(km):
    return np.asarray(km.seq_coll.forward_sba), np.asarray(km.kmer_sba_start_indices).copy()


def force(monkeypatch, path):
    if path == "auto":
        monkeypatch.delitem(_native.options, "GKM_LCP_PATH", raising=False)
    else:
        monkeypatch.setitem(_native.options, "GKM_LCP_PATH", path)


# ---------------------------------------------------------------------------------------------
# the check of one sorted object
# ---------------------------------------------------------------------------------------------
def premise(ref, cap, n):
    """not trivial: the values 0 and cap, at least three between them, and some k-mer not unique"""
    values = np.unique(ref)
    assert values[0] == 0 and values[-1] == cap, (values[:3], values[-3:], cap)
    assert ((values > 0) & (values < cap)).sum() >= 3, values
    assert lcpref.spectrum(ref, cap)[1][cap] < n


def check(km, cap, monkeypatch, paths, mult_lens=(), default_cap=False):
    """lcp, spectrum and min_unique on each path, then the multiplicity tracks, against lcpref; -> the
    reference array."""
    sba, st = host_view(km)
    n = len(st)
    ref = lcpref.lcp(sba, st, cap)
    premise(ref, cap, n)
    want_distinct, want_unique = lcpref.spectrum(ref, cap)
    want_track = lcpref.min_unique_track(len(sba), st, ref, cap)
    args = () if default_cap else (cap,)
    for path in paths:
        force(monkeypatch, path)
        got = km.lcp(*args)
        assert got.dtype == np.uint32 and got.shape == (n,), path
        np.testing.assert_array_equal(got, ref, err_msg=path)
        distinct, unique = km.kmer_spectrum(*args)
        assert distinct.dtype == np.int64 and unique.dtype == np.int64, path
        np.testing.assert_array_equal(distinct, want_distinct, err_msg=path)
        np.testing.assert_array_equal(unique, want_unique, err_msg=path)
        track = km.min_unique_lengths(*args)
        assert track.dtype == np.uint32 and track.shape == (len(sba),), path
        np.testing.assert_array_equal(track, want_track, err_msg=path)
    force(monkeypatch, "auto")
    for k in mult_lens:
        at = km.max_kmer_len if k is None else k  # the default is the sort length (None: whole suffixes)
        want = lcpref.multiplicity_track(sba, st, at, lcp_arr=ref if at is not None and at <= cap else None)
        np.testing.assert_array_equal(km.multiplicity_track(k), want, err_msg=f"kmer_len = {k}")
    return ref


def paths_for(seqs, kmin, kmax):
    return ("auto", "keys", "bytes") if keys_eligible(seqs, kmin, kmax) else ("auto", "bytes")


def check_keys_refused(km, monkeypatch):
    force(monkeypatch, "keys")
    with pytest.raises(_native.GkError, match="GKM_LCP_PATH=keys") as e:
        km.lcp(3)
    assert e.value.code == _native.GK_E_UNSUPPORTED
    force(monkeypatch, "auto")


# ---------------------------------------------------------------------------------------------
# 1. the sweep: every LCP value, across the key words' edges
# ---------------------------------------------------------------------------------------------
# 2-bit keys hold 32 symbols a word: 31 | 32 | 33 and 63 | 64 | 65 cross the first two word edges on
# W = 1, 2, 3; 96 fills W = 3, 97 and 100 need W = 4.  4-bit keys hold 16: 16 | 17 the first edge, 31, 33, 49 and 64 on W = 2..4.
@pytest.mark.parametrize("k", [31, 32, 33, 63, 64, 65, 96, 97, 100])
def test_sweep_acgt(k, monkeypatch):
    seqs = sweep_seqs(k)
    km = sorted_kmers(seqs, k, k)
    assert km._engine.key_layout() == ((2 * k + 63) // 64, 2, k)
    ref = check(km, k, monkeypatch, ("auto", "keys", "bytes"), mult_lens=(None, k, min(k - 1, 40), 1), default_cap=True)
    assert set(range(k + 1)) <= set(ref.tolist()), "the sweep must give every LCP value"


@pytest.mark.parametrize("k", [16, 17, 31, 33, 49, 64])
def test_sweep_iupac(k, monkeypatch):
    seqs = sweep_seqs(k + 100, tails="NRYKM")
    km = sorted_kmers(seqs, k, k)
    assert km._engine.key_layout() == ((4 * k + 63) // 64, 4, k)
    ref = check(km, k, monkeypatch, ("auto", "keys", "bytes"), mult_lens=(k, k // 2), default_cap=True)
    assert set(range(k + 1)) <= set(ref.tolist())


def test_sweep_caps_below_the_sort_length(monkeypatch):
    """caps inside every key word of a three-word key, through both paths"""
    seqs = sweep_seqs(7)
    km = sorted_kmers(seqs, 96, 96)
    for cap in (5, 32, 33, 64, 65, 95):
        check(km, cap, monkeypatch, ("keys", "bytes"))


# ---------------------------------------------------------------------------------------------
# 2. tile edges: an equal pair, a differing pair and the last element on each side of an edge
# ---------------------------------------------------------------------------------------------
# (edge E, what sits there, seed, copies, n): the LCP kernel reads the key of position E - 1 for
# position E from the lane below or, at a wave's first lane, by a halo load; the spectrum and the
# min_unique track read lcp[E] for position E - 1 from the lane above or a halo load; the
# multiplicity track's flag scan has tiles of SCAN_TILE flags.  "equal": lcp[E] == cap (a group spans
# the edge), "differs": lcp[E] < cap and lcp[E - 1] == cap or lcp[E + 1] == cap (a group ends or
# starts at the edge), "last-before": n == E (position E - 1 is the last: lcp[n] = 0 is read at the
# edge), "last-after": n == E + 1 (one element in the last tile).
EDGE_CASES = [
    (TILE, "equal", 1, 10, TILE + 300), (TILE, "differs", 7, 10, TILE + 300),
    (TILE, "last-before", 1, 10, TILE), (TILE, "last-after", 1, 10, TILE + 1),
    (2 * TILE, "equal", 2, 30, 2 * TILE + 700), (2 * TILE, "differs", 9, 30, 2 * TILE + 700),
    (2 * TILE, "last-before", 1, 20, 2 * TILE), (2 * TILE, "last-after", 1, 20, 2 * TILE + 1),
    (SCAN_TILE, "equal", 1, 60, SCAN_TILE + 900), (SCAN_TILE, "differs", 8, 60, SCAN_TILE + 900),
    (SCAN_TILE, "last-before", 1, 50, SCAN_TILE), (SCAN_TILE, "last-after", 1, 50, SCAN_TILE + 1),
    (TILE - 64, "equal", 2, 10, TILE + 300), (TILE + THREADS, "differs", 14, 10, TILE + 300),
]


@pytest.mark.parametrize("edge,what,seed,copies,n", EDGE_CASES, ids=[f"{c[0]}-{c[1]}" for c in EDGE_CASES])
def test_tile_edges(edge, what, seed, copies, n, monkeypatch):
    K = 31
    seqs = edge_seqs(seed, copies, K, n)
    km = sorted_kmers(seqs, K, K)
    assert len(km) == n
    sba, st = host_view(km)
    ref = lcpref.lcp(sba, st, K)
    if what == "equal":
        assert ref[edge] == K and ref[edge - 1] == K
    elif what == "differs":
        assert ref[edge] < K and (ref[edge - 1] == K or ref[edge + 1] == K)
    else:
        assert n == edge + (what == "last-after") and ref[n - 1] < K
    check(km, K, monkeypatch, ("keys", "bytes"), mult_lens=(K, 12, 4))


# ---------------------------------------------------------------------------------------------
# 3. orders the byte path serves
# ---------------------------------------------------------------------------------------------
GOLDEN_BYTE_CASES = [("iupac_k31", 31), ("iupac_min6_max25", 25), ("iupac_suffix_min2", 12), ("repeat_k31", 31),
                     ("repeat_k40", 40), ("repeat_min10_max40", 40), ("repeat_suffix_min4", 40),
                     ("repeat_suffix_min4", 12)]


@pytest.mark.parametrize("name,cap", GOLDEN_BYTE_CASES, ids=[f"{n}-cap{c}" for n, c in GOLDEN_BYTE_CASES])
def test_golden_orders(name, cap, monkeypatch):
    """the manifest's mixed-alphabet and repeat cases: direct 4-bit keys, bounded 2-bit keys with a
    length field (bytes only), suffix orders with max_len 12 and 40 (rank keys: bytes only)"""
    case, seqs = CASES[name], golden_seqs(name)
    kmin, kmax = case["min_kmer_len"], case["max_kmer_len"]
    km = sorted_kmers(seqs, kmin, kmax)
    np.testing.assert_array_equal(km.kmer_sba_start_indices, load_case(name)["starts_stable"])
    check(km, cap, monkeypatch, paths_for(seqs, kmin, kmax), mult_lens=(kmax, cap, max(cap // 3, kmin)),
          default_cap=kmax is not None)
    if not keys_eligible(seqs, kmin, kmax):
        check_keys_refused(km, monkeypatch)


def test_equal_short_tails(monkeypatch):
    """min < max on A/C/G/T (keys with a length field: the byte path): two contigs end in the same
    bases, so two k-mers cut short by the '$' are equal at every length -- lcp == cap, between k-mers
    shorter than cap."""
    tail = "GATTACAC"
    seqs = [("a", rand_seq(1, 300) + tail), ("b", rand_seq(2, 280) + tail), ("c", rand_seq(3, 150))]
    kmin, cap = 2, 9
    km = sorted_kmers(seqs, kmin, cap)
    sba, st = host_view(km)
    ref = lcpref.lcp(sba, st, cap)
    dollars = np.append(np.flatnonzero(sba == 36), len(sba))
    left = dollars[np.searchsorted(dollars, st)] - st  # bases before the '$' / the end
    assert ((left < cap) & (ref == cap)).sum() >= len(tail) - kmin, "equal short k-mers must exist"
    assert ((left < cap) & (ref < left)).any()
    check(km, cap, monkeypatch, ("auto", "bytes"), mult_lens=(cap, 5, 2), default_cap=True)
    check_keys_refused(km, monkeypatch)


@pytest.mark.parametrize("kmin,kmax,cap,option", [(10, 40, 40, {"GKM_MSD_KEYS_MIN": "2"}), (130, 130, 130, {}),
                                                  (130, 130, 77, {}), (4, None, 64, {"GKM_MSD_KEYS_MIN": "2"})],
                         ids=["capped-doubling-10-40", "ranks-k130", "ranks-k130-cap77", "suffix-doubling-groups"])
def test_rank_key_orders(kmin, kmax, cap, option, monkeypatch):
    """sorts that went through prefix doubling: the keys are ranks (or stale behind them), so the bytes
    decide; the 400-base repeat keeps k-mers equal up to every cap used"""
    for name, value in option.items():
        monkeypatch.setitem(_native.options, name, value)
    rep = rand_seq(50, 400)
    seqs = [("a", rand_seq(51, 2000) + rep + rand_seq(52, 700)), ("b", rand_seq(53, 300) + rep + rand_seq(54, 301) + rep)]
    km = sorted_kmers(seqs, kmin, kmax)
    check(km, cap, monkeypatch, ("auto", "bytes"), mult_lens=(kmax, cap, 20), default_cap=kmax == cap)
    check_keys_refused(km, monkeypatch)


def test_assigned_start_subset(monkeypatch):
    """a user-assigned subset of the starts, sorted: the arrays cover the subset, and track positions
    outside it hold 0"""
    K = 24
    seqs = sweep_seqs(5, copies=60) + [("r", rand_seq(6, 3000))]
    sc = SequenceCollection(sequence_list=seqs, strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K, max_kmer_len=K)
    every = np.asarray(km.kmer_sba_start_indices)
    keep = np.random.default_rng(9).random(len(every)) < 0.6
    subset = every[keep][::-1].copy()  # (descending: the sort does not rely on the given order)
    km.kmer_sba_start_indices = subset
    km.sort()
    assert len(km) == len(subset) < len(every)
    check(km, K, monkeypatch, paths_for(seqs, K, K), mult_lens=(K, 9), default_cap=True)
    outside = np.ones(len(sc.forward_sba), dtype=bool)
    outside[subset] = False
    assert outside[every].any()
    for track in (km.min_unique_lengths(), km.multiplicity_track(), km.multiplicity_track(9)):
        assert not track[outside].any() and track[subset].all()


# ---------------------------------------------------------------------------------------------
# 4. the spectrum's bins
# ---------------------------------------------------------------------------------------------
def test_spectrum_bins_beyond_lds(monkeypatch):
    """suffix order of a 3,000-base contig, a copy of it and a copy that differs in its last base, at
    max_len 2500: the suffixes of the first two are equal to their '$' (lcp == cap: one global bin
    takes thousands of counts) and those of the third give every value up to the cap once (the bins
    past the LDS ones, one count each)"""
    cap = 2500
    a = rand_seq(77, 3000)
    seqs = [("a", a), ("b", a), ("c", a[:-1] + chr(NEXT[ord(a[-1])]))]
    km = sorted_kmers(seqs, 1, None)
    ref = check(km, cap, monkeypatch, ("auto", "bytes"), mult_lens=(None, cap, LDS_BINS))
    assert cap > 2 * LDS_BINS and (ref == cap).sum() > 3000
    assert len(np.unique(ref[ref >= LDS_BINS])) > 1000
    # a cap below the LDS bin count is served from the same view
    check(km, LDS_BINS - 1, monkeypatch, ("auto",))
    check(km, LDS_BINS, monkeypatch, ("auto",))


@pytest.mark.parametrize("cap", [64, 2000])
def test_spectrum_one_bin(cap, monkeypatch):
    """a poly-A contig of 5,000 bases in suffix order: neighbours A^i and A^(i+1) share i bases, so all
    but the first cap k-mers sit on the bin cap -- every lane of nearly every wave on one bin, in LDS
    (cap 64) and in global memory (cap 2000)"""
    km = sorted_kmers([("a", "A" * 5000)], 1, None)
    ref = check(km, cap, monkeypatch, ("auto", "bytes"), mult_lens=(None, cap, 3))
    assert (ref == cap).sum() == 5000 - cap


# ---------------------------------------------------------------------------------------------
# 5. past the grid cap
# ---------------------------------------------------------------------------------------------
LARGE_BASES = 4_300_000


@pytest.fixture(scope="module")
def large():
    """One 4,300,000-base A/C/G/T contig with a 60 k segment copied twice, sorted at 31 (the group
    tests' size): more k-mers than GRID_CAP tiles of TILE, so every kernel strides; the reference
    array is computed once."""
    rng = np.random.default_rng(43)
    sba = ACGT[rng.integers(0, 4, LARGE_BASES)].copy()
    sba[1_000_000:1_060_000] = sba[:60_000]
    sba[3_000_000:3_060_000] = sba[:60_000]
    km = sorted_kmers([("c0", sba.tobytes().decode())], 31, 31)
    _, st = host_view(km)
    assert len(st) == LARGE_BASES - 30 > GRID_CAP * TILE
    ref = lcpref.lcp(sba, st, 31)
    premise(ref, 31, len(st))
    return km, sba, st, ref


@pytest.mark.parametrize("path", ["keys", "bytes"])
def test_large_lcp_spectrum_and_min_unique(large, path, monkeypatch):
    km, sba, st, ref = large
    force(monkeypatch, path)
    np.testing.assert_array_equal(km.lcp(), ref)
    distinct, unique = km.kmer_spectrum()
    want_distinct, want_unique = lcpref.spectrum(ref, 31)
    np.testing.assert_array_equal(distinct, want_distinct)
    np.testing.assert_array_equal(unique, want_unique)
    np.testing.assert_array_equal(km.min_unique_lengths(), lcpref.min_unique_track(len(sba), st, ref, 31))
    assert unique[31] < distinct[31] < len(st) and distinct[12] > 1 << 20


@pytest.mark.parametrize("k", [31, 12])
def test_large_multiplicity(large, k):
    """at the sort length (the sort's own heads) and at 12 (masked keys): more than 1025 scan tiles"""
    km, sba, st, ref = large
    want = lcpref.multiplicity_track(sba, st, k, lcp_arr=ref)
    assert want.max() >= 3 and len(st) > 1025 * SCAN_TILE
    np.testing.assert_array_equal(km.multiplicity_track(k), want)


# ---------------------------------------------------------------------------------------------
# 6. the extreme keys, the existing calls, canonical orders
# ---------------------------------------------------------------------------------------------
def test_keys_zero_and_all_ones(monkeypatch):
    """poly-A and poly-T 32-mers: the keys 0 and 2^64 - 1, each several times, first and last of the order"""
    seqs = [("a", "A" * 40), ("t", "T" * 40)] + sweep_seqs(11, copies=40)
    km = sorted_kmers(seqs, 32, 32)
    keys = km.get_encoded_kmers()[:, 0]
    assert (keys[:9] == 0).all() and (keys[-9:] == np.uint64(2**64 - 1)).all()
    ref = check(km, 32, monkeypatch, ("auto", "keys", "bytes"), mult_lens=(32, 31, 1), default_cap=True)
    assert (ref[1:9] == 32).all() and (ref[-8:] == 32).all() and ref[9] < 32 and ref[-9] < 32


def test_agrees_with_the_group_calls():
    """distinct[k] and unique[k] are the group count and the count of groups of one that
    get_kmer_group_counts(k) reports; the multiplicity track at K is np.repeat of the unique view's
    counts scattered to the starts"""
    K = 31
    seqs = golden_seqs("repeat_k31")
    km = sorted_kmers(seqs, K, K)
    distinct, unique = km.kmer_spectrum()
    for k in (1, 7, K):
        hist, total = km.get_kmer_group_counts(k)
        assert total == len(km)
        assert (distinct[k], unique[k]) == (hist.sum(), hist[1]), k
    _, counts = km.get_unique_kmers()
    assert counts.max() > 1
    st = np.asarray(km.kmer_sba_start_indices)
    np.testing.assert_array_equal(km.multiplicity_track(K)[st], np.repeat(counts, counts))
    np.testing.assert_array_equal(km.multiplicity_track()[st], np.repeat(counts, counts))


def revcomp(b: bytes) -> bytes:
    return b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_canonical_order():
    """groups exist at the sort length, so the multiplicity track does; everything that needs
    prefixes is refused"""
    K = 21
    a = rand_seq(31, 1500)
    seqs = [("a", a), ("b", revcomp(a[200:900].encode()).decode() + rand_seq(32, 300))]
    km = sorted_kmers(seqs, K, K, canonical=True)
    sba, st = host_view(km)
    raw = sba.tobytes()

    def canon(p):
        w = raw[p:p + K]
        return min(w, revcomp(w))

    counts = Counter(canon(int(p)) for p in st)
    want = np.zeros(len(sba), dtype=np.uint32)
    for p in st.tolist():
        want[p] = counts[canon(p)]
    assert want.max() >= 2 and (want[st] == 1).any()
    np.testing.assert_array_equal(km.multiplicity_track(), want)
    np.testing.assert_array_equal(km.multiplicity_track(K), want)
    for call in (km.lcp, km.kmer_spectrum, km.min_unique_lengths, lambda: km.multiplicity_track(10)):
        with pytest.raises(_native.GkError, match="canonical") as e:
            call()
        assert e.value.code == _native.GK_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# 7. the cached view
# ---------------------------------------------------------------------------------------------
def builds(engine) -> int:
    rep = engine.profile_report()
    return sum(rep.get(name, {"count": 0})["count"] for name in ("lcp_keys", "lcp_bytes"))


def test_view_is_cached_and_rebuilt():
    K = 31
    seqs = sweep_seqs(21) + [("r", rand_seq(22, 2000))]
    km = sorted_kmers(seqs, K, K)
    sba, st = host_view(km)
    ref = lcpref.lcp(sba, st, K)
    premise(ref, K, len(st))
    eng = km._engine
    eng.profile_enable(True)
    np.testing.assert_array_equal(km.lcp(31), ref)
    assert builds(eng) == 1
    # a smaller cap is served from the view by clamping: the array, the spectrum, the track
    np.testing.assert_array_equal(km.lcp(10), np.minimum(ref, 10))
    distinct, unique = km.kmer_spectrum(10)
    np.testing.assert_array_equal(distinct, lcpref.spectrum(ref, 10)[0])
    np.testing.assert_array_equal(unique, lcpref.spectrum(ref, 10)[1])
    np.testing.assert_array_equal(km.min_unique_lengths(10), lcpref.min_unique_track(len(sba), st, ref, 10))
    np.testing.assert_array_equal(km.lcp(), ref)
    assert builds(eng) == 1
    # a multiplicity track (a group pass) leaves the view alone
    np.testing.assert_array_equal(km.multiplicity_track(12), lcpref.multiplicity_track(sba, st, 12, lcp_arr=ref))
    np.testing.assert_array_equal(km.lcp(31), ref)
    assert builds(eng) == 1
    # a new sort drops it; a small cap first, then a larger one: rebuilt and correct
    km.sort()
    np.testing.assert_array_equal(km.kmer_sba_start_indices, st)
    np.testing.assert_array_equal(km.lcp(10), np.minimum(ref, 10))
    assert builds(eng) == 2
    np.testing.assert_array_equal(km.lcp(31), ref)
    assert builds(eng) == 3
    np.testing.assert_array_equal(km.kmer_spectrum(31)[0], lcpref.spectrum(ref, 31)[0])
    assert builds(eng) == 3
    eng.profile_enable(False)


def test_view_is_not_reused_after_a_sort_at_another_length():
    sba = np.frombuffer("$".join(s for _, s in sweep_seqs(23, copies=50)).encode(), dtype=np.uint8)
    e = _native.Engine()
    e.set_sequence(sba, np.concatenate([[0], np.flatnonzero(sba == 36) + 1]).astype(np.uint32))
    e.enumerate(20)
    e.sort(31)
    st31 = e.copy_starts()
    np.testing.assert_array_equal(e.lcp(31), lcpref.lcp(sba, st31, 31))
    e.sort(20)
    st20 = e.copy_starts()
    assert not np.array_equal(st20, st31)
    want = lcpref.lcp(sba, st20, 20)
    premise(want, 20, len(st20))
    np.testing.assert_array_equal(e.lcp(20), want)
    with pytest.raises(_native.GkError, match="above the sort length") as err:
        e.lcp(31)
    assert err.value.code == _native.GK_E_ARG
    # new starts: no view, no sort
    e.enumerate(20)
    for call in (lambda: e.lcp(20), lambda: e.lcp_spectrum(20), lambda: e.position_track(1, 20, len(sba)),
                 lambda: e.position_track(2, 0, len(sba))):
        with pytest.raises(_native.GkError, match="not sorted") as err:
            call()
        assert err.value.code == _native.GK_E_STATE


def test_other_queries_are_unchanged():
    """find, compare and screen on the same object give the same answers before and after"""
    K = 31
    seqs_a = sweep_seqs(24) + [("r", rand_seq(25, 3000))]
    seqs_b = sweep_seqs(24, copies=30) + [("r", rand_seq(26, 3000))]
    km, other = sorted_kmers(seqs_a, K, K), sorted_kmers(seqs_b, K, K)
    queries = [seqs_a[0][1][40:40 + K], seqs_a[5][1][3:3 + K], "A" * K, seqs_a[-1][1][100:100 + K]]
    reads = [seqs_a[3][1], seqs_b[-1][1][:500], "ACGT" * 20]

    def answers():
        first, count = km.find(queries)
        scr = km.screen(reads)
        return first.tolist(), count.tolist(), km.compare(other), scr.n_present.tolist(), scr.occurrences.tolist()

    before = answers()
    assert sum(before[1]) > 3 and before[2]["n_shared"] > 0 and sum(before[3]) > 0
    km.lcp()
    km.kmer_spectrum(12)
    km.min_unique_lengths()
    assert answers() == before
    km.multiplicity_track()
    km.multiplicity_track(8)
    assert answers() == before


# ---------------------------------------------------------------------------------------------
# 8. preconditions on the device side
# ---------------------------------------------------------------------------------------------
def test_preconditions():
    seqs = sweep_seqs(27, copies=30)
    km = sorted_kmers(seqs, 31, 31)
    e, L = km._engine, len(km.seq_coll.forward_sba)
    lib = e.lib
    assert lib.gk_copy_lcp(e.ctx, 0, None, 0) == _native.GK_E_STATE  # no view yet
    assert lib.gk_device_lcp(e.ctx, None, None) == _native.GK_E_STATE
    assert lib.gk_device_track(e.ctx, None, None) == _native.GK_E_STATE
    for call, code, text in [
            (lambda: e.lcp(0), _native.GK_E_ARG, "max_len must be >= 1"),
            (lambda: e.lcp_spectrum(0), _native.GK_E_ARG, "max_len must be >= 1"),
            (lambda: e.lcp(32), _native.GK_E_ARG, "above the sort length"),
            (lambda: e.position_track(_native.TRACK_MIN_UNIQUE, 0, L), _native.GK_E_ARG, "max_len must be >= 1"),
            (lambda: e.position_track(_native.TRACK_MULTIPLICITY, 32, L), _native.GK_E_ARG, "above the sort length"),
            (lambda: e.position_track(3, 31, L), _native.GK_E_ARG, "kind"),
            (lambda: e.position_track(_native.TRACK_MIN_UNIQUE, 31, L + 1), _native.GK_E_ARG, "sba_len"),
            (lambda: e.position_track(_native.TRACK_MULTIPLICITY, 31, L - 1), _native.GK_E_ARG, "sba_len")]:
        with pytest.raises(_native.GkError, match=text) as err:
            call()
        assert err.value.code == code, text
    assert lib.gk_lcp_spectrum(e.ctx, 31, None, None) == _native.GK_E_ARG
    n = len(km)
    got = e.lcp(31)
    part = np.empty(5, dtype=np.uint32)
    assert lib.gk_copy_lcp(e.ctx, n - 5, part.ctypes.data_as(_native._U32P), 5) == _native.GK_OK
    np.testing.assert_array_equal(part, got[-5:])
    assert lib.gk_copy_lcp(e.ctx, n - 4, part.ctypes.data_as(_native._U32P), 5) == _native.GK_E_ARG
    assert e.device_lcp()[1] == n and e.device_lcp()[0]
    e.position_track(_native.TRACK_MULTIPLICITY, 0, L)
    assert e.device_track()[1] == L and e.device_track()[0]
    # a suffix order takes any cap up to 2^24
    sfx = sorted_kmers(seqs, 3, None)
    with pytest.raises(_native.GkError, match="above 2\\^24") as err:
        sfx._engine.lcp((1 << 24) + 1)
    assert err.value.code == _native.GK_E_ARG
    with pytest.raises(ValueError, match="needs max_len when max_kmer_len is None"):
        sfx.lcp()
    # fewer than two k-mers: no keys, the byte path, lcp == [0]
    one = sorted_kmers([("a", "ACGTACGTAC")], 10, 10)
    assert one.lcp().tolist() == [0] and one.kmer_spectrum(3)[0].tolist() == [0, 1, 1, 1]
    assert one.min_unique_lengths().tolist() == [1] + [0] * 9 and one.multiplicity_track().tolist() == [1] + [0] * 9
