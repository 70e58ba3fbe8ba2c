"""Minimizer sampling on the device: gk_minimizers through _native.Engine.minimizers and
Kmers.minimizers, gk_select_minimizers through Kmers.select_minimizers, and Kmers.find_minimizers.

Every expectation comes from tests/minimizerref.py (numpy: the definition by windows; the local rule for
the one large input) and never from the code under test.  Every parametrised case first asserts on that
reference alone that it is not trivial -- 0 < selected < valid starts -- but for the designed
all-selected and none-selected cases.  pos, keys, strands and the per-read counts are compared exactly.
T mirrors the kernel's tile (gkm_minimizer.hip: kMzThreads threads of kMzRounds positions each).
"""

from functools import lru_cache

import numpy as np
import pytest

import minimizerref as ref
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection

pytestmark = pytest.mark.gpu

T = 256 * 4  # kMzTile
CANON, LEX = _native.MINIMIZER_CANONICAL, _native.MINIMIZER_LEX
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


@lru_cache(maxsize=None)
def engine():
    return _native.Engine()


def rnd(seed, n, letters=b"ACGT") -> bytes:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes()


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def n_valid(arr, off, k):
    return int(ref.position_keys(arr, off, k, False)[0].sum())


def flags_of(canonical, lex):
    return (CANON if canonical else 0) | (LEX if lex else 0)


def assert_same(got, want, note=""):
    for g, w_, name, dtype in zip(got, want, ("pos", "key", "strand", "per_seq"),
                                  (np.uint64, np.uint64, np.uint8, np.uint32)):
        assert g.dtype == dtype, (note, name)
        np.testing.assert_array_equal(g, w_, err_msg=f"{note} {name}")


def check(seqs, k, w, canonical=False, lex=False, trivial=None, local=False, note=""):
    """The device's answer for the batch against the reference's; returns the reference's."""
    arr, off = ref.as_batch(seqs)
    want = (ref.by_local_rule if local else ref.by_windows)(arr, off, k, w, canonical, lex)
    nv = n_valid(arr, off, k)
    if trivial is None:
        assert 0 < want[0].size < nv, (note, want[0].size, nv)
    elif trivial == "all":
        assert want[0].size == nv > 0, note
    else:
        assert want[0].size == 0, note
    got = engine().minimizers((arr, off), k, w, flags_of(canonical, lex))
    assert_same(got, want, f"{note} k={k} w={w} canonical={canonical} lex={lex}")
    return want


# ---------------------------------------------------------------------------------------------
# the k x w x order x canonical grid
# ---------------------------------------------------------------------------------------------
KS = (1, 3, 15, 16, 31, 32)
WS = (1, 2, 10, 19, 64, 256)


@lru_cache(maxsize=None)
def grid_batch():
    a = bytearray(rnd(1, 3000))
    a[700] = a[701] = ord("N")
    a[2200] = ord("R")
    return [bytes(a), rnd(2, 1500), rnd(3, 40), b"", rnd(4, 700), rnd(5, 2100)]


def grid_cases():
    out = []
    for i, k in enumerate(KS):
        for j, w in enumerate(WS):
            combos = [((i + j) & 1, ((i + j) >> 1) & 1)]
            if k in (1, 32) and w in (2, 19, 256):  # the edge lengths under every combination
                combos = [(0, 0), (0, 1), (1, 0), (1, 1)]
            out += [(k, w, bool(c), bool(x)) for c, x in combos]
    return out


@pytest.mark.parametrize("k,w,canonical,lex", grid_cases())
def test_grid(k, w, canonical, lex):
    check(grid_batch(), k, w, canonical, lex, trivial="all" if w == 1 else None)


@pytest.mark.parametrize("lex", (False, True))
@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("w", (10, 64))
def test_least_and_greatest_key(w, canonical, lex):
    """k = 32: the all-A 32-mer is key 0, the all-T one key 2^64 - 1 (canonical: key 0, strand 1)."""
    seqs = [rnd(6, 1500) + b"A" * 600 + rnd(7, 700) + b"T" * 600 + rnd(8, 900)]
    _, key, strand, _ = check(seqs, 32, w, canonical, lex)
    assert (key == 0).any()
    if canonical:
        assert ((key == 0) & (strand == 1)).any() and ((key == 0) & (strand == 0)).any()
    else:
        assert (key == np.uint64(2**64 - 1)).any()


# ---------------------------------------------------------------------------------------------
# sweeps across the tile edge, +-(w + k) positions
# ---------------------------------------------------------------------------------------------
SWEEPS = ((4, 8, False), (15, 19, False), (2, 5, True))  # (k, w, lex)


def sweep_of(k, w):
    return range(-(w + k), w + k + 1)


@pytest.mark.parametrize("k,w,lex", SWEEPS)
def test_read_boundary_across_the_tile_edge(k, w, lex):
    body = rnd(10, 2 * T + 700)
    for d in sweep_of(k, w):
        check([body[:T + d], body[T + d:]], k, w, lex=lex, note=f"boundary at T{d:+d}")
        check([body[:T + d], b"", b"", body[T + d:]], k, w, canonical=True, lex=lex, note=f"empty reads at T{d:+d}")


@pytest.mark.parametrize("k,w,lex", SWEEPS)
def test_single_n_across_the_tile_edge(k, w, lex):
    body = rnd(11, 2 * T + 300)
    for d in sweep_of(k, w):
        s = bytearray(body)
        s[T + d] = ord("N")
        check([bytes(s)], k, w, lex=lex, note=f"N at T{d:+d}")


@pytest.mark.parametrize("k,w,lex", SWEEPS)
def test_batch_end_across_the_tile_edge(k, w, lex):
    body = rnd(12, T + 100)
    for d in sweep_of(k, w):
        check([body[:T + d]], k, w, lex=lex, note=f"end at T{d:+d}")
        check([body[:300], body[300:T + d]], k, w, canonical=True, lex=lex, note=f"two reads, end at T{d:+d}")


@pytest.mark.parametrize("k,w", ((4, 8), (15, 19), (1, 64)))
def test_lone_least_kmer_across_the_tile_edge(k, w):
    """Lexicographic order over a background without A: the only all-A k-mer wins every window it is in."""
    body = rnd(13, 2 * T + 300, b"CGT")
    for d in sweep_of(k, w):
        s = bytearray(body)
        s[T + d:T + d + k] = b"A" * k
        pos = check([bytes(s)], k, w, lex=True, note=f"least at T{d:+d}")[0]
        assert T + d in pos.tolist()


@pytest.mark.parametrize("k,w", ((1, 8), (4, 8), (6, 19), (15, 64)))
def test_tie_goes_left_across_the_tile_edge(k, w):
    """Two equal k-mers one window apart (p and p + w - 1), a smaller one right behind the second: the
    window that holds both takes the left one, and every other window of the second holds the smaller
    k-mer.  So the second is never selected -- also when the two sit in different tiles."""
    assert w >= k + 2
    body = rnd(14, 2 * T + 300, b"GT")
    for d in sweep_of(k, w):
        p = T + d - (w - 1) // 2  # the pair straddles position T + d
        q = p + w - 1
        s = bytearray(body)
        s[p:p + k + 1] = b"C" * k + b"G"
        s[q:q + k + 1] = b"C" * k + b"A"
        pos = check([bytes(s)], k, w, lex=True, note=f"pair around T{d:+d}")[0].tolist()
        assert p in pos and q not in pos and q + 1 in pos


# ---------------------------------------------------------------------------------------------
# tied runs longer than two tiles
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lex", (False, True))
@pytest.mark.parametrize("w", (10, 256))
def test_poly_a_run(w, lex):
    k, run = 15, 2 * T + 500
    head, tail = rnd(15, 333), rnd(16, 700)
    pos = check([head + b"A" * run + tail], k, w, lex=lex)[0]
    # every all-A start with a full window of all-A starts to its right is selected
    first, last = len(head), len(head) + run - k  # the all-A starts
    inside = set(pos.tolist())
    assert all(p in inside for p in range(first, last - (w - 1) + 1))


@pytest.mark.parametrize("unit", (b"AC", b"ACG", b"AACGT"))
@pytest.mark.parametrize("k,w,canonical,lex", ((15, 10, False, False), (16, 64, True, False), (31, 256, False, True),
                                               (3, 256, True, True)))
def test_periodic_repeats(unit, k, w, canonical, lex):
    reps = (2 * T + 700) // len(unit)
    check([rnd(17, 100) + unit * reps + rnd(18, 611), unit * 400], k, w, canonical, lex)


# ---------------------------------------------------------------------------------------------
# run and read shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", ((1, 2), (3, 10), (15, 19), (32, 64), (5, 256)))
def test_runs_of_w_minus_one_w_and_w_plus_one(k, w):
    def run_of(seed, starts):
        return rnd(seed, starts + k - 1)

    for starts, trivial in ((w - 1, "none"), (w, None), (w + 1, None)):
        one = [run_of(20, starts)]
        assert n_valid(*ref.as_batch(one), k) == starts
        pos = check(one, k, w, trivial=trivial, note=f"one run of {starts}")[0]
        assert pos.size == (0, 1)[starts - w + 1] if starts <= w else pos.size in (1, 2)
    # the three runs in one read, separated by single N's, and as three reads
    runs = [run_of(21, w - 1), run_of(22, w), run_of(23, w + 1)]
    check([b"N".join(runs)], k, w, note="N-separated runs")
    res = check(runs, k, w, note="runs as reads")
    assert res[3][0] == 0 and res[3][1] >= 1 and res[3][2] >= 1


def test_reads_shorter_than_k_and_empty_reads():
    k, w = 15, 4
    seqs = [b"", rnd(30, 14), rnd(31, 15), b"", b"", rnd(32, 17), rnd(33, 18), rnd(34, 400), b"", rnd(35, 3), b""]
    res = check(seqs, k, w)
    assert res[3].tolist()[:7] == [0, 0, 0, 0, 0, 0, 1]  # (18 bases: 4 starts, the first full window)
    check([b"", b"", b""], k, w, trivial="none")
    check([rnd(36, 14)] * 5, k, w, trivial="none")
    # nseq == 0
    pos, key, strand, per_seq = engine().minimizers((np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)), k, w, 0)
    assert pos.size == key.size == strand.size == per_seq.size == 0


@pytest.mark.parametrize("k,w", ((1, 2), (2, 3)))
def test_more_read_ends_in_a_tile_than_256(k, w):
    """700 reads of 0 to 4 bases inside two tiles (the screen kernel's LDS table holds 256 ends a pass; this
    kernel keeps none), then 300 empty reads and a long one."""
    rng = np.random.default_rng(40)
    lens = rng.integers(0, 5, 700).tolist()
    seqs = [rnd(41 + i, n) for i, n in enumerate(lens)] + [b""] * 300 + [rnd(39, 1500)] + [b""] * 5
    assert sum(lens) < 2 * T and (np.cumsum(lens) < T).sum() > 256
    check(seqs, k, w, lex=True)
    check(seqs, k, w, canonical=True)


def test_a_read_longer_than_three_tiles():
    for k, w, canonical in ((31, 19, True), (16, 256, False)):
        check([rnd(50, 77), rnd(51, 3 * T + 555), rnd(52, 90)], k, w, canonical)


# ---------------------------------------------------------------------------------------------
# canonical keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 8, 12))
def test_even_k_palindromes_have_strand_zero(k):
    seqs = [rnd(60, 500) + b"ACGT" * 40 + rnd(61, 300) + b"AATT" * 30 + rnd(62, 200)]
    for w in (1, 3):
        pos, key, strand, _ = check(seqs, k, w, canonical=True, lex=True, trivial="all" if w == 1 else None)
        own_rc = np.array([ref.revcomp_key(int(x), k) == int(x) for x in key])
        assert own_rc.sum() > 10 and not strand[own_rc].any() and strand.any()


def test_reverse_complemented_batch_has_the_same_keys_per_read():
    k, w = 15, 10
    reads = [rnd(70 + i, n) for i, n in enumerate((300, 800, 24, 33, 1500, 0, 650))]
    rc = [revcomp(r) for r in reads]
    fw_ref = check(reads, k, w, canonical=True)
    rc_ref = check(rc, k, w, canonical=True)

    def per_read(res):
        ends = np.cumsum(res[3])
        return [np.sort(res[1][e - c:e]).tolist() for e, c in zip(ends.tolist(), res[3].tolist())]

    # (on the reference alone: random 15-mers do not tie inside a window, so mirroring keeps the choice)
    assert per_read(fw_ref) == per_read(rc_ref) and sum(map(len, per_read(fw_ref))) > 100
    arr_f, off_f = ref.as_batch(reads)
    arr_r, off_r = ref.as_batch(rc)
    got_f = engine().minimizers((arr_f, off_f), k, w, CANON)
    got_r = engine().minimizers((arr_r, off_r), k, w, CANON)
    assert per_read(got_f) == per_read(got_r)
    # a mirrored minimizer sits at len - k - pos and has the other strand unless it is its own reverse complement
    assert (got_f[2].sum() + got_r[2].sum()) == got_f[2].size


# ---------------------------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------------------------
def test_chunk_ends_swept_through_both_halos(monkeypatch):
    k, w = 5, 7
    seqs = [rnd(80, 900), rnd(81, 1300), b"", rnd(82, 40), rnd(83, 1100)]
    arr, off = ref.as_batch(seqs)
    want = ref.by_windows(arr, off, k, w, True, False)
    assert 0 < want[0].size < n_valid(arr, off, k)
    for chunk in range(T - 2 * (w + k), T + 2 * (w + k) + 1):
        monkeypatch.setitem(_native.options, "GKM_MINIMIZER_CHUNK", str(chunk))
        assert_same(engine().minimizers((arr, off), k, w, CANON), want, f"chunk {chunk}")
    for chunk in range(1, 2 * (w + k)):  # chunks shorter than a halo
        monkeypatch.setitem(_native.options, "GKM_MINIMIZER_CHUNK", str(chunk * 13))
        assert_same(engine().minimizers((arr, off), k, w, CANON), want, f"chunk {chunk * 13}")


@pytest.mark.parametrize("k,w,canonical,lex", ((15, 10, False, False), (31, 256, True, False), (1, 64, False, True)))
def test_same_result_for_three_chunk_sizes_and_again(monkeypatch, k, w, canonical, lex):
    seqs = [rnd(85, 5000), b"A" * 1200, rnd(86, 3000) + b"N" + rnd(87, 2500), rnd(88, 10)]
    arr, off = ref.as_batch(seqs)
    want = ref.by_windows(arr, off, k, w, canonical, lex)
    assert 0 < want[0].size < n_valid(arr, off, k)
    for chunk in ("997", "1024", "4099", None, None):
        if chunk is None:
            monkeypatch.delitem(_native.options, "GKM_MINIMIZER_CHUNK", raising=False)
        else:
            monkeypatch.setitem(_native.options, "GKM_MINIMIZER_CHUNK", chunk)
        assert_same(engine().minimizers((arr, off), k, w, flags_of(canonical, lex)), want, f"chunk {chunk}")


def test_a_batch_of_4_3_million_bases():
    """More tiles than any launch above; the reference by the local rule."""
    rng = np.random.default_rng(90)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4_300_000)].copy()
    body[rng.integers(0, body.size, 300)] = ord("N")
    body[1_000_000:1_003_000] = ord("A")
    cuts = np.sort(rng.integers(0, body.size, 4000))
    off = np.concatenate([[0], cuts, [body.size]]).astype(np.uint64)
    want = ref.by_local_rule(body, off, 15, 5)
    assert 0 < want[0].size < n_valid(body, off, 15)
    assert_same(engine().minimizers((body, off), 15, 5, 0), want, "4.3 M bases")


# ---------------------------------------------------------------------------------------------
# the Python layer: MinimizerResult
# ---------------------------------------------------------------------------------------------
def small_genome():
    return [("c0", rnd(100, 5000).decode()), ("c1", rnd(101, 1200).decode())]


def test_kmers_minimizers_result():
    sc = SequenceCollection(sequence_list=small_genome(), strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=15, max_kmer_len=15)
    reads = [rnd(110, 400), b"", rnd(111, 20) + b"N" + rnd(112, 90), rnd(113, 700)]
    arr, off = ref.as_batch(reads)
    for kwargs, k, w, canonical, lex in (({"w": 10}, 15, 10, False, False),
                                         ({"w": 4, "kmer_len": 7, "canonical": True, "order": "lex"}, 7, 4, True, True)):
        pos, key, strand, per_seq = ref.by_windows(arr, off, k, w, canonical, lex)
        assert 0 < pos.size < n_valid(arr, off, k)
        res = km.minimizers([r.decode() for r in reads], **kwargs)
        assert isinstance(res, gk.MinimizerResult)
        assert res.offsets.dtype == np.int64 and res.pos.dtype == np.uint32
        assert res.keys.dtype == np.uint64 and res.strands.dtype == np.uint8
        np.testing.assert_array_equal(res.offsets, np.concatenate([[0], np.cumsum(per_seq)]))
        np.testing.assert_array_equal(res.pos, pos - np.repeat(off[:-1], per_seq))
        np.testing.assert_array_equal(res.keys, key)
        np.testing.assert_array_equal(res.strands, strand)
    packed = km.minimizers((arr, off), 10)  # an already packed batch
    np.testing.assert_array_equal(packed.keys, ref.by_windows(arr, off, 15, 10)[1])
    assert not km._is_sorted and km._minimizer_spec is None  # (nothing of the k-mer set changed)


# ---------------------------------------------------------------------------------------------
# select_minimizers: the genome's minimizers as the start set
# ---------------------------------------------------------------------------------------------
PALINDROME = "ACGTACGTACGT"


@lru_cache(maxsize=None)
def genome(name):
    """"acgt": random contigs with a poly-A region, a segment that occurs twice, palindromes, an all-T contig
    and a contig shorter than w + k - 1.  "mixed": N runs and IUPAC letters beside random contigs."""
    def r(seed, n):
        return rnd(seed, n).decode()

    if name == "acgt":
        a, b, c = r(120, 12000), r(121, 9000), r(122, 8000)
        main = a + "A" * 200 + b + PALINDROME + a[3000:3700] + c + PALINDROME + r(123, 500)
        return [("main", main), ("polyT", "T" * 70), ("short", r(124, 23)), ("tail", r(125, 900))]
    if name == "mixed":
        x = r(126, 9000)
        return [("m0", r(127, 3000) + "N" * 40 + r(128, 2500) + "RYKM" + r(129, 800) + "N" + r(130, 700)),
                ("m1", x), ("m2", x[2000:2600] + "NNNNNNNNNNNNNNNN" + r(131, 3000) + "W" + x[100:400]),
                ("short", r(132, 21))]
    raise KeyError(name)


def fresh_kmers(name, k):
    sc = SequenceCollection(sequence_list=genome(name), strands_to_load="forward")
    return gk.Kmers(sc, min_kmer_len=k, max_kmer_len=k), sc


def sba_reference(sba, k, w, canonical=False, lex=False):
    sba = np.asarray(sba, dtype=np.uint8)
    return ref.by_windows(sba, np.array([0, sba.size], dtype=np.uint64), k, w, canonical, lex)


@pytest.mark.parametrize("name,k,w,canonical,order", (("acgt", 15, 10, False, "hash"), ("acgt", 21, 11, True, "hash"),
                                                      ("mixed", 15, 10, False, "lex"), ("mixed", 12, 12, True, "hash"),
                                                      ("acgt", 15, 1, False, "hash")))
def test_select_minimizers_start_set_and_find(name, k, w, canonical, order):
    km, sc = fresh_kmers(name, k)
    sba = np.asarray(sc.forward_sba)
    assert (sba == ord("$")).sum() == len(genome(name)) - 1
    pos, key, strand, _ = sba_reference(sba, k, w, canonical, order == "lex")
    nv = n_valid(sba, np.array([0, sba.size], dtype=np.uint64), k)
    assert (pos.size == nv) if w == 1 else (0 < pos.size < nv)
    short = [s for _, s in genome(name) if len(s) < w + k - 1]
    assert w == 1 or (short and all(len(s) >= k for s in short))
    n = km.select_minimizers(w, canonical=canonical, order=order)
    assert n == pos.size == len(km) and not km._is_sorted and km._minimizer_spec == (w, canonical, order)
    starts = km.kmer_sba_start_indices
    assert starts.dtype == np.uint32
    np.testing.assert_array_equal(starts, pos.astype(np.uint32))
    km.sort(canonical=canonical)
    # find of every selected k-mer: the count np.unique gives over the selected (canonical) k-mers
    uniq, counts = np.unique(key, return_counts=True)
    windows = sba[pos.astype(np.int64)[:, None] + np.arange(k)[None, :]]
    _, count = km.find(np.ascontiguousarray(windows))
    np.testing.assert_array_equal(count, counts[np.searchsorted(uniq, key)])
    assert counts.max() > 1
    if w > 1:
        # k-mers that occur in the genome and are never selected: count 0
        valid, ckey, _, _ = ref.position_keys(sba, np.array([0, sba.size], dtype=np.uint64), k, canonical)
        never = np.flatnonzero(valid & ~np.isin(ckey, uniq))[:500]
        assert never.size > 100
        _, count = km.find(np.ascontiguousarray(sba[never[:, None] + np.arange(k)[None, :]]))
        assert not count.any()
    # the sorted sampled index is the sort of the assigned subset
    km2, _ = fresh_kmers(name, k)
    km2.kmer_sba_start_indices = pos.astype(np.uint32)
    km2.sort(canonical=canonical)
    np.testing.assert_array_equal(km.kmer_sba_start_indices, km2.kmer_sba_start_indices)
    assert km2._minimizer_spec is None


def test_select_minimizers_with_a_contig_shorter_than_k():
    """At the engine: Kmers refuses a min_kmer_len above the shortest contig."""
    k, w = 15, 6
    contigs = [rnd(140, 3000), rnd(141, 9), rnd(142, 14), rnd(143, 15), rnd(144, 19), rnd(145, 20), rnd(146, 2000)]
    sba = np.frombuffer(b"$".join(contigs), dtype=np.uint8)
    seg = np.cumsum([0] + [len(c) + 1 for c in contigs[:-1]]).astype(np.uint32)
    eng = _native.Engine()
    eng.set_sequence(sba, seg)
    for flags in (0, CANON | LEX):
        pos = sba_reference(sba, k, w, bool(flags & CANON), bool(flags & LEX))[0]
        inside = [int(((pos >= s) & (pos < s + len(c))).sum()) for s, c in zip(seg.tolist(), contigs)]
        assert inside[1:5] == [0, 0, 0, 0] and inside[5] >= 1 and inside[0] > 100  # (20 bases: one window)
        assert eng.select_minimizers(k, w, flags) == pos.size
        np.testing.assert_array_equal(eng.copy_starts(), pos.astype(np.uint32))


# ---------------------------------------------------------------------------------------------
# end to end: reads against the sampled index
# ---------------------------------------------------------------------------------------------
K2, W2 = 15, 10


@lru_cache(maxsize=None)
def sampled_index(canonical):
    km, sc = fresh_kmers("mixed", K2)
    km.select_minimizers(W2, canonical=canonical)
    km.sort(canonical=canonical)
    return km, sc


def cut_reads(sc, seed, n_reads=40, length=150):
    """Forward reads from ACGT-only stretches of the genome: (start in the sba, bytes)."""
    sba = np.asarray(sc.forward_sba)
    ok = np.isin(sba, np.frombuffer(b"ACGT", dtype=np.uint8))
    run = np.zeros(sba.size + 1, dtype=np.int64)  # ACGT bytes in a row from each position on
    for p in range(sba.size - 1, -1, -1):
        run[p] = run[p + 1] + 1 if ok[p] else 0
    cand = np.flatnonzero(run[:-1] >= length)
    rng = np.random.default_rng(seed)
    starts = rng.choice(cand, n_reads, replace=False)
    assert length >= W2 + K2 - 1
    return [(int(s), sba[s:s + length].tobytes()) for s in starts]


def test_forward_reads_find_their_origin():
    km, sc = sampled_index(False)
    reads = cut_reads(sc, 150)
    res, first, count = km.find_minimizers([r for _, r in reads])
    arr, off = ref.as_batch([r for _, r in reads])
    want = ref.by_windows(arr, off, K2, W2)
    np.testing.assert_array_equal(res.keys, want[1])
    np.testing.assert_array_equal(np.diff(res.offsets), want[3])
    assert res.pos.size >= len(reads) and (count >= 1).all()
    starts = km.kmer_sba_start_indices
    for j, (origin, read) in enumerate(reads):
        for i in range(int(res.offsets[j]), int(res.offsets[j + 1])):
            where = starts[int(first[i]):int(first[i]) + int(count[i])]
            assert origin + int(res.pos[i]) in where.tolist()
    # the same through get_kmer_locations, for the first read's minimizers
    origin, read = reads[0]
    names = [n for n, _ in genome("mixed")]
    seg_starts = np.asarray(sc._forward_sba_seg_starts).astype(np.int64)
    for i in range(int(res.offsets[0]), int(res.offsets[1])):
        p = int(res.pos[i])
        at = origin + p
        seg = int(np.searchsorted(seg_starts, at, side="right")) - 1
        locs = km.get_kmer_locations(read[p:p + K2])
        assert ("+", names[seg], at - int(seg_starts[seg])) in locs


def test_reverse_complemented_reads_against_a_canonical_selection():
    km, sc = sampled_index(True)
    reads = [revcomp(r) for _, r in cut_reads(sc, 151)]
    res, first, count = km.find_minimizers(reads)
    arr, off = ref.as_batch(reads)
    want = ref.by_windows(arr, off, K2, W2, canonical=True)
    np.testing.assert_array_equal(res.keys, want[1])
    np.testing.assert_array_equal(res.strands, want[2])
    assert res.pos.size >= len(reads) and (count >= 1).all()


def test_reads_with_substitutions_lose_some_minimizers():
    km, sc = sampled_index(False)
    reads = []
    rng = np.random.default_rng(152)
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    for _, r in cut_reads(sc, 153):
        s = bytearray(r)
        for p in np.flatnonzero(rng.integers(0, 25, len(s)) == 0).tolist():
            s[p] = nxt[s[p]]
        reads.append(bytes(s))
    arr, off = ref.as_batch(reads)
    want = ref.by_windows(arr, off, K2, W2)
    sba = np.asarray(sc.forward_sba)
    gkeys, gcounts = np.unique(sba_reference(sba, K2, W2)[1], return_counts=True)
    at = np.searchsorted(gkeys, want[1])
    at_c = np.minimum(at, gkeys.size - 1)
    present = gkeys[at_c] == want[1]
    expect = np.where(present, gcounts[at_c], 0).astype(np.uint32)
    assert 0 < (expect == 0).sum() < expect.size  # on the reference alone: some are absent, some present
    res, _, count = km.find_minimizers(reads)
    np.testing.assert_array_equal(res.keys, want[1])
    np.testing.assert_array_equal(count, expect)


# ---------------------------------------------------------------------------------------------
# lifetime and preconditions
# ---------------------------------------------------------------------------------------------
def test_view_is_replaced_by_a_second_call():
    eng = _native.Engine()
    a = ref.as_batch([rnd(160, 3000)])
    b = ref.as_batch([rnd(161, 500), rnd(162, 40)])
    lib = eng.lib
    import ctypes
    assert lib.gk_copy_minimizers(eng.ctx, None, None, None, 0) == _native.GK_E_STATE
    assert lib.gk_device_minimizers(eng.ctx, None, None, None, None) == _native.GK_E_STATE
    first = eng.minimizers(a, 15, 10, 0)
    p1 = eng.device_minimizers()
    assert p1[3] == first[0].size > 0 and p1[0] and p1[1] and p1[2]
    second = eng.minimizers(b, 7, 3, CANON)
    assert eng.device_minimizers()[3] == second[0].size != first[0].size
    assert_same(second, ref.by_windows(*b, 7, 3, True, False))
    # n must be the view's count; each array may be NULL
    pos = np.zeros(second[0].size + 1, dtype=np.uint64)
    ptr = pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.gk_copy_minimizers(eng.ctx, ptr, None, None, second[0].size + 1) == _native.GK_E_ARG
    assert lib.gk_copy_minimizers(eng.ctx, ptr, None, None, first[0].size) == _native.GK_E_ARG
    assert lib.gk_copy_minimizers(eng.ctx, ptr, None, None, second[0].size) == _native.GK_OK
    np.testing.assert_array_equal(pos[:-1], second[0])
    assert lib.gk_copy_minimizers(eng.ctx, None, None, None, second[0].size) == _native.GK_OK
    # an empty batch leaves an empty view
    empty = eng.minimizers((np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64)), 15, 10, 0)
    assert empty[0].size == 0 and empty[3].tolist() == [0, 0] and eng.device_minimizers()[3] == 0


def test_sort_join_and_lcp_survive_minimizers_and_select_drops_them():
    km, _ = fresh_kmers("acgt", 15)
    other, _ = fresh_kmers("acgt", 15)
    km.sort()
    other.sort()
    sorted_starts = km.kmer_sba_start_indices.copy()
    lcp = km.lcp()
    joined = km.count_in(other)
    res = km.minimizers([rnd(170, 2500)], 10)
    assert res.pos.size > 0
    assert km._is_sorted
    np.testing.assert_array_equal(km._engine.copy_starts(), sorted_starts)
    assert km._engine.device_lcp()[1] == lcp.size
    again = km._engine.join_result()
    np.testing.assert_array_equal(again[0], joined[0])
    np.testing.assert_array_equal(again[1], joined[1])
    np.testing.assert_array_equal(km.lcp(), lcp)
    n = km.select_minimizers(10)
    assert 0 < n < sorted_starts.size and not km._is_sorted
    with pytest.raises(_native.GkError) as e:
        km._engine.device_lcp()
    assert e.value.code == _native.GK_E_STATE
    with pytest.raises(_native.GkError) as e:
        km._engine.join_result()
    assert e.value.code == _native.GK_E_STATE
    with pytest.raises(AssertionError, match="must be sorted"):
        km.find("ACGTACGTACGTACG")
    # lcp and count_in on the sampled index, as on any assigned subset
    km.sort()
    km2, _ = fresh_kmers("acgt", 15)
    km2.kmer_sba_start_indices = np.sort(km.kmer_sba_start_indices)
    km2.sort()
    np.testing.assert_array_equal(km.lcp(), km2.lcp())
    a, b = km.count_in(other), km2.count_in(other)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_argument_and_state_errors():
    import ctypes
    eng = _native.Engine()
    lib = eng.lib
    arr, off = ref.as_batch([rnd(180, 100), rnd(181, 50)])
    n = ctypes.c_uint64(7)
    ap = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def call(offsets=off, nseq=2, k=15, w=10, flags=0, seqs=ap, n_out=ctypes.byref(n)):
        op = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64).ctypes.data_as(
            ctypes.POINTER(ctypes.c_uint64))
        return lib.gk_minimizers(eng.ctx, seqs, op, nseq, k, w, flags, n_out, None)

    assert call() == _native.GK_OK
    kept = n.value
    assert kept == ref.by_windows(arr, off, 15, 10)[0].size > 0
    for kwargs, text in (({"k": 0}, "k = 0"), ({"k": 33}, "k = 33"), ({"w": 0}, "w = 0"), ({"w": 257}, "w = 257"),
                         ({"flags": 4}, "flags = 4"), ({"flags": 0x80000001}, "unknown flag bits"),
                         ({"offsets": None}, "null offsets"), ({"seqs": None}, "null seqs"), ({"n_out": None}, "null n_out"),
                         ({"offsets": [1, 100, 150]}, "offsets[0] must be 0"),
                         ({"offsets": [0, 100, 90]}, "offsets decrease at sequence 1"),
                         # (the offsets are judged before any byte is read: no 4 GiB array is needed)
                         ({"offsets": [0, 100, 100 + 2**32]}, "sequence 1 is longer than 2^32 - 1 bytes")):
        assert call(**kwargs) == _native.GK_E_ARG, kwargs
        assert text in lib.gk_last_error(eng.ctx).decode(), kwargs
    # a call refused for its arguments has touched nothing: the earlier view is still there
    assert eng.device_minimizers()[3] == kept
    assert lib.gk_minimizers(eng.ctx, None, None, 0, 15, 10, 0, ctypes.byref(n), None) == _native.GK_OK and n.value == 0
    # gk_select_minimizers: arguments, then the state
    for k, w, flags in ((0, 10, 0), (33, 10, 0), (15, 0, 0), (15, 257, 0), (15, 10, 8)):
        assert lib.gk_select_minimizers(eng.ctx, k, w, flags, None) == _native.GK_E_ARG
    assert lib.gk_select_minimizers(eng.ctx, 15, 10, 0, None) == _native.GK_E_STATE
    assert "no sequence loaded" in lib.gk_last_error(eng.ctx).decode()


def test_python_layer_errors():
    km, _ = fresh_kmers("acgt", 15)
    with pytest.raises(ValueError, match="chosen by select_minimizers"):
        km.find_minimizers("ACGT" * 10)
    km.select_minimizers(10, canonical=True)
    with pytest.raises(ValueError, match=r"needs sort\(canonical=True\)"):
        km.find_minimizers("ACGT" * 10)
    km.sort()
    with pytest.raises(ValueError, match=r"needs sort\(canonical=True\)"):
        km.find_minimizers("ACGT" * 10)
    km.sort(canonical=True)
    res, first, count = km.find_minimizers(["ACGT" * 10, "ACG"])
    assert res.offsets.size == 3 and first.size == count.size == res.pos.size
    res, first, count = km.find_minimizers(["ACG", ""])  # no minimizer at all
    assert res.pos.size == first.size == count.size == 0 and res.offsets.tolist() == [0, 0, 0]
    km.kmer_sba_start_indices = np.arange(100, dtype=np.uint32)  # the setter forgets the spec
    with pytest.raises(ValueError, match="chosen by select_minimizers"):
        km.find_minimizers("ACGT" * 10)
    km.select_minimizers(4)
    assert km._minimizer_spec == (4, False, "hash")
    km._initialize()  # re-initialisation forgets it too
    assert km._minimizer_spec is None and len(km) == sum(len(s) - 14 for _, s in genome("acgt"))
    wide, _ = fresh_kmers("acgt", 20)
    wide.max_kmer_len = None
    with pytest.raises(ValueError, match="select_minimizers needs min_kmer_len == max_kmer_len"):
        wide.select_minimizers(10)
