"""Pin tests/edgegen.py (the edge-aimed sort inputs) before tests/test_gpu_sort_edges.py relies on
it: where every '$', run and single letter lies relative to the tile, and how many k-mers of each
class a planted run makes -- from the arrays alone and oracle.enumerate_starts.  CPU only.
"""

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import edgegen
from oracle import oracle

DOLLAR = edgegen.DOLLAR
TILES = [4096, 8192, 18432, 24576]
KS = [3, 4, 8, 10, 16, 17, 24, 31, 32, 33, 55, 56, 57, 63, 64]
IS_ACGT = np.zeros(256, dtype=bool)
IS_ACGT[np.frombuffer(b"ACGT", dtype=np.uint8)] = True


def contig_bounds(sba, seg):
    """[(first, one past the last base)] of every contig"""
    seg = seg.astype(np.int64)
    return list(zip(seg.tolist(), np.append(seg[1:] - 1, len(sba)).tolist()))


def check_layout(label, sba, seg, k, acgt_only):
    assert sba.dtype == np.uint8 and seg.dtype == np.uint32, label
    np.testing.assert_array_equal(seg, edgegen.segments_of(sba), err_msg=label)
    for b, e in contig_bounds(sba, seg):
        assert e - b >= k, (label, b, e)
    rest = sba[sba != DOLLAR]
    assert IS_ACGT[rest].all() == acgt_only, label


def tied_kmers(sba, seg, k):
    """the number of k-mers that have an equal k-mer elsewhere in the array"""
    starts = oracle.enumerate_starts(sba, seg, k)
    _, inverse, counts = np.unique(sliding_window_view(sba, k)[starts], axis=0, return_inverse=True,
                                   return_counts=True)
    return int((counts[inverse.ravel()] > 1).sum())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TILES)
def test_ends_lengths_and_kmer_counts(T):
    for k in KS:
        got = edgegen.ends(k, T)
        want = list(dict.fromkeys([T - 1, T, T + 1, T + k - 2, T + k - 1, T + k, 2 * T - k + 1, 2 * T, 2 * T + 7,
                                   2 * T + k - 1]))
        assert [len(s) for _, s, _ in got] == want
        assert [lab for lab, _, _ in got] == [f"ends-L{L}" for L in want]
        n = []
        for label, sba, seg in got:
            check_layout(label, sba, seg, k, acgt_only=True)
            assert seg.tolist() == [0] and not (sba == DOLLAR).any()
            starts = oracle.enumerate_starts(sba, seg, k)
            np.testing.assert_array_equal(starts, np.arange(len(sba) - k + 1))
            n.append(len(starts))
        # exactly one and two tiles of k-mers, one less and one more (0 and 2 k-mers beside the full tile)
        assert {T - 1, T, T + 1, 2 * T} <= set(n)
        # the last tile holds 1 and 2 k-mers, the halo of the first ends 0, 1 and 2 bases behind it
        assert {n_ % T for n_ in n} >= {0, 1, T - 1}


@pytest.mark.parametrize("T", TILES)
def test_separator_positions(T):
    for k in KS:
        got = {lab: (s, g) for lab, s, g in edgegen.separators(k, T)}
        offsets = [-k - 1, -k, -k + 1, -1, 0, 1, k - 1, k]
        assert len(set(offsets)) == 8
        assert len(got) == 2 * 8 + 4
        for m in (1, 2):
            for d in offsets:
                label = f"sep-{m}T{d:+d}"
                sba, seg = got[label]
                check_layout(label, sba, seg, k, acgt_only=True)
                at = m * T + d
                assert np.flatnonzero(sba == DOLLAR).tolist() == [at], label
                assert seg.tolist() == [0, at + 1], label
                starts = oracle.enumerate_starts(sba, seg, k).astype(np.int64)
                first, second = starts[starts < at], starts[starts > at]
                assert first.max() + k - 1 == at - 1 and second.min() == at + 1, label
                if d == 0:  # the last k-mer of the first contig ends on the last position of a tile
                    assert (first.max() + k) % T == 0, label
                if d == -1:  # the first k-mer of the second contig starts on the first position of a tile
                    assert second.min() % T == 0, label
                if d == k:  # the k-mer on the tile's last position keeps its whole window (all halo)
                    assert m * T - 1 in first and m * T in first, label
                if d == k - 1:  # ... the next one, on the tile's first position, loses its last base
                    assert first.max() == m * T - 1, label
        for o in (-k, -k + 1, -1, 0):
            label = f"exact-T{o:+d}"
            sba, seg = got[label]
            check_layout(label, sba, seg, k, acgt_only=True)
            assert np.flatnonzero(sba == DOLLAR).tolist() == [T + o - 1] and len(sba) == T + o + k, label
            starts = oracle.enumerate_starts(sba, seg, k).astype(np.int64)
            assert starts[starts >= T + o - 1].tolist() == [T + o], label  # one k-mer: the contig itself
            np.testing.assert_array_equal(sba[T + o:], sba[T // 4:T // 4 + k], err_msg=label)


def test_comb_covers_every_residue():
    for k in KS:
        (label, sba, seg), = edgegen.comb(k)
        check_layout(label, sba, seg, k, acgt_only=True)
        dollars = np.flatnonzero(sba == DOLLAR)
        np.testing.assert_array_equal(dollars, 129 * np.arange(1, 65) - 1)
        assert len(sba) == 65 * 128 + 64
        for mod in (8, 32, 64):
            assert set((dollars % mod).tolist()) == set(range(mod))
        # never two stops in one 64-position row (hence 32-position word, 8-position window)
        assert len(set((dollars // 64).tolist())) == 64 and (np.diff(dollars) == 129).all()
        assert [e - b for b, e in contig_bounds(sba, seg)] == [128] * 65


@pytest.mark.parametrize("B", [24576, 65536])
def test_tails_lengths_mod_32(B):
    for k in (31, 32, 57):
        got = edgegen.tails(k, B)
        assert [len(s) % 32 for _, s, _ in got] == [0, 1, 31, 31, 31]
        assert [len(s) for _, s, _ in got[:3]] == [B, B + 1, B + 31]
        for (label, sba, seg), at in zip(got[3:], (B - 1, B)):
            assert np.flatnonzero(sba == DOLLAR).tolist() == [at], label
        for label, sba, seg in got:
            check_layout(label, sba, seg, k, acgt_only=True)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4, 16, 17, 31, 32, 33, 56, 57, 63])
@pytest.mark.parametrize("T", [8192, 24576])
def test_runs_layout_and_class_b_counts(k, T):
    """Every planted run makes max(0, n - k + 1) homopolymer k-mers, and every k-mer of its contig
    that overlaps it without lying inside is a non-homopolymer class-B k-mer."""
    plans = edgegen.runs_plan(k, T)
    arrays = edgegen.runs(k, T)
    assert [p["label"] for p in plans] == [lab for lab, _, _ in arrays]
    labels = [p["label"] for p in plans]
    lengths = edgegen.run_lengths(k)
    assert lengths == [n for n in (k - 1, k, k + 1, 32 + k - 1, 64 + k)]
    for n in lengths:
        assert f"fixed-a-n{n}" in labels and f"fixed-b-n{n}" in labels
    for p, (label, sba, seg) in zip(plans, arrays):
        check_layout(label, sba, seg, k, acgt_only=False)
        assert len(sba) == p["L"] and 3 * T < len(sba) <= 3 * T + T // 4 + 13
        np.testing.assert_array_equal(np.flatnonzero(sba == DOLLAR), sorted(p["dollars"]))
        # nothing but the plan is outside ACGT
        planted = np.zeros(len(sba), dtype=bool)
        for a, n, c in p["runs"]:
            assert (sba[a:a + n] == c).all(), (label, a)
            planted[a:a + n] = True
        for a, c in p["singles"]:
            assert sba[a] == c, (label, a)
            planted[a] = True
        planted[p["dollars"]] = True
        np.testing.assert_array_equal(~IS_ACGT[sba], planted, err_msg=label)
        starts = oracle.enumerate_starts(sba, seg, k).astype(np.int64)
        win = sliding_window_view(sba, k)[starts]
        class_b = (~IS_ACGT[win]).any(axis=1)
        homo = (win == win[:, :1]).all(axis=1) & class_b
        bounds = contig_bounds(sba, seg)
        for a, n, c in p["runs"]:
            b, e = next((b, e) for b, e in bounds if b <= a < e)
            assert a + n <= e, (label, a)
            lo, hi = max(a - k + 1, b), min(a + n - 1, e - k)  # the starts whose window overlaps the run
            sel = (starts >= lo) & (starts <= hi)
            assert sel.sum() == hi - lo + 1 and class_b[sel].all(), (label, a)
            assert homo[sel].sum() == max(0, n - k + 1), (label, a, n)
            if n >= k:
                np.testing.assert_array_equal(starts[sel][homo[sel]], np.arange(a, a + n - k + 1), err_msg=label)


@pytest.mark.parametrize("T", [8192, 24576])
def test_runs_placements(T):
    k = 31
    plans = {p["label"]: p for p in edgegen.runs_plan(k, T)}
    for n in edgegen.run_lengths(k):
        a, b = plans[f"fixed-a-n{n}"], plans[f"fixed-b-n{n}"]
        firsts_a = [r[0] for r in a["runs"]]
        assert firsts_a == [0, T - n, 2 * T, a["dollars"][0] - n, a["L"] - n]  # at 0, ending on T - 1, ..., the last byte
        assert [r[0] for r in b["runs"]] == [b["dollars"][0] + 1, T, 2 * T - n]
    # every split straddles T, 2 T and 3 T with some run length, every run length straddles with every split
    seen = set()
    for s in edgegen.RUN_SPLITS:
        edges = set()
        for h in (0, 1):
            for a, n, _ in plans[f"straddle-s{s}-{h}"]["runs"]:
                E = a + s
                assert E % T == 0 and a < E < a + n
                edges.add(E // T)
                seen.add((n, s))
        if s < min(edgegen.run_lengths(k)):
            assert edges == {1, 2, 3}
    # (a run no longer than the split cannot straddle)
    assert seen == {(n, s) for n in edgegen.run_lengths(k) for s in edgegen.RUN_SPLITS if n > s}
    singles = {pos for lab in ("letters-a", "letters-b") for pos, _ in plans[lab]["singles"]}
    assert {T - 1, T, T + 31, T + 32} <= singles
    for lab in ("letters-a", "letters-b"):
        p = plans[lab]
        ends_ = [p["dollars"][0], p["L"]]
        assert all(any(e - k <= pos < e for pos, _ in p["singles"]) for e in ends_), lab
    p = plans["last-k-only"]
    assert p["runs"] == [] and len(p["singles"]) == 1 and p["L"] - (k - 1) <= p["singles"][0][0] < p["L"]
    ry = plans["complement-ry"]["runs"]
    assert {c for _, _, c in ry} == {ord("R"), ord("Y")}
    assert any(a < T < a + n for a, n, _ in ry) and any(a < 2 * T < a + n for a, n, _ in ry)


def test_runs_subsets_keep_the_labels():
    full = {lab: s for lab, s, _ in edgegen.runs(31, 8192)}
    part = edgegen.runs(31, 8192, lengths=(32,), splits=(17,), extras=False)
    assert [lab for lab, _, _ in part] == ["fixed-a-n32", "fixed-b-n32", "straddle-s17-0"]
    assert len(full) == 10 + 10 + 4


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 31, 57])
def test_every_array_has_planted_ties(k):
    """The repeat of 3 k bases gives at least 2 (2 k + 1) tied k-mers (k = 4 ties by chance as well);
    comb's contigs hold min(3 k, 128) of it."""
    T = 4096
    for label, sba, seg in edgegen.ends(k, T) + edgegen.separators(k, T) + edgegen.runs(k, T) + edgegen.tails(k, T):
        assert tied_kmers(sba, seg, k) >= 2 * (2 * k + 1), label
    (label, sba, seg), = edgegen.comb(k)
    assert tied_kmers(sba, seg, k) >= 2 * (min(3 * k, 128) - k + 1), label


def test_builders_are_deterministic():
    for build in (lambda: edgegen.ends(31, 4096), lambda: edgegen.separators(31, 4096), lambda: edgegen.comb(31),
                  lambda: edgegen.runs(31, 4096), lambda: edgegen.tails(31, 4096)):
        for (la, sa, ga), (lb, sb, gb) in zip(build(), build()):
            assert la == lb and np.array_equal(sa, sb) and np.array_equal(ga, gb)


# ---------------------------------------------------------------------------------------------
# the builders for the variable-length and suffix-order sorts
# ---------------------------------------------------------------------------------------------
def longest_run(sba, letter):
    """(first, length) of the longest run of `letter`"""
    is_l = np.concatenate([[0], (sba == letter).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(is_l))
    firsts, lengths = edges[0::2], edges[1::2] - edges[0::2]
    i = int(lengths.argmax())
    return int(firsts[i]), int(lengths[i])


@pytest.mark.parametrize("k", [1, 3, 5, 40, 125])
def test_long_ties_layout(k):
    got = {lab: (s, g) for lab, s, g in edgegen.long_ties(k)}
    assert list(got) == ["polyA-6000", "period8", "polyA-cross"]
    want = {"polyA-6000": (13002, [3500, 9501]), "period8": (12002, [2000, 10001]), "polyA-cross": (10802, [4000, 8301])}
    for label, (sba, seg) in got.items():
        check_layout(label, sba, seg, k, acgt_only=True)
        L, dollars = want[label]
        assert len(sba) == L and 10_000 <= L <= 13_002, label
        assert np.flatnonzero(sba == DOLLAR).tolist() == dollars, label
        r = min(3 * k, 600)
        np.testing.assert_array_equal(sba[100:100 + r], sba[dollars[1] + 101:dollars[1] + 101 + r], err_msg=label)
    # the poly-A contigs are whole contigs: a '$' (or nothing) on both sides
    sba, _ = got["polyA-6000"]
    assert longest_run(sba, ord("A")) == (3501, 6000) and (sba[3501:9501] == ord("A")).all()
    sba, _ = got["polyA-cross"]
    first, n = longest_run(sba, ord("A"))
    assert (first, n) == (4001, 4300)
    assert first < 4096 < 8192 < first + n  # it crosses both positions
    assert (first - 1, first + n) == (4000, 8301)  # ... from '$' to '$'
    sba, _ = got["period8"]
    np.testing.assert_array_equal(sba[2001:10001], np.tile(np.frombuffer(b"ACGTTGCA", dtype=np.uint8), 1000))
    # nothing tied is longer than the 6,000 bases the oracle's cost was measured at
    assert max(n for _, plan in edgegen.long_ties_plan() for kind, n in plan if kind == "A") == 6000


@pytest.mark.parametrize("k,tails", [(1, edgegen.TAILS_ACGT), (5, edgegen.TAILS_ACGT), (40, edgegen.TAILS_ACGT),
                                     (3, edgegen.TAILS_IUPAC)])
def test_shared_tails_layout(k, tails):
    assert edgegen.TAILS_ACGT == (700, 28, 29, 30) and edgegen.TAILS_IUPAC == (700, 15, 16, 17)
    got = edgegen.shared_tails(k, tails)
    assert [lab for lab, _, _ in got] == [f"tail{n}" for n in tails] + [f"tail{n}-lone" for n in tails[1:]]
    positions = edgegen.tail_positions(k, tails)
    for (label, sba, seg), n in zip(got[len(tails):], tails[1:]):
        # one end contig (the first), the two inside contigs, 'A', 'C', 'G' before their tails
        check_layout(label, sba, seg, k, acgt_only=True)
        assert 10_000 <= len(sba) <= 13_000, (label, len(sba))
        assert [e - b for b, e in contig_bounds(sba, seg)] == [2000, 1600 + n, 1600 + n, 4500, 600], label
        pos = positions[label]
        assert pos == [2000 - n, 2001 + 800, 2001 + 1601 + n + 800], label
        assert all((sba[q:q + n] == sba[pos[0]:pos[0] + n]).all() for q in pos), label
        assert sba[pos[0] + n] == DOLLAR and [chr(sba[q + n]) for q in pos[1:]] == ["T", "C"], label
        assert [chr(sba[q - 1]) for q in pos] == ["A", "C", "G"], label
    for (label, sba, seg), n in zip(got[:len(tails)], tails):
        check_layout(label, sba, seg, k, acgt_only=True)
        assert 10_000 <= len(sba) <= 13_000, (label, len(sba))
        bounds = contig_bounds(sba, seg)
        lengths = [e - b for b, e in bounds]
        exact = [n] if n >= k else []
        assert lengths == [2000] + exact + [1600 + n, 1600 + n, 2500, 1800, 600], label
        pos = positions[label]
        assert len(pos) == len(bounds) - 1 and pos == sorted(pos), label
        tail = sba[pos[0]:pos[0] + n]
        ends_here, inside = [], []
        for q in pos:
            np.testing.assert_array_equal(sba[q:q + n], tail, err_msg=f"{label} at {q}")
            b, e = next((b, e) for b, e in bounds if b <= q < e)
            (ends_here if q + n == e else inside).append((q, b, e))
        # three contigs end in the tail (the first of the array among them: the tail's lowest position
        # has exactly n bases to its '$'), one is the tail, two hold it inside
        assert len(ends_here) == 3 + len(exact) and len(inside) == 2, label
        assert ends_here[0][0] == pos[0] == 2000 - n, label
        if exact:
            assert any(q == b and e - b == n for q, b, e in ends_here), label
        # behind the inside tails: 'T' first, 'C' second -- the later position sorts first
        assert [chr(sba[q + n]) for q, _, _ in inside] == ["T", "C"] and inside[0][0] < inside[1][0], label
        assert all(q - b == 800 and e - q - n == 800 for q, b, e in inside), label


@pytest.mark.parametrize("builder,k,T", [("ends", 5, 4096), ("ends", 125, 4096), ("separators", 3, 4096),
                                         ("separators", 65, 4096), ("separators", 1, 12288), ("comb", 3, None),
                                         ("comb", 125, None), ("long_ties", 3, None), ("shared_tails", 3, None)])
def test_iupac_variant_keeps_edges_and_copies(builder, k, T):
    args = (k,) if T is None else (k, T)
    kw = {"tails": edgegen.TAILS_IUPAC} if builder == "shared_tails" else {}
    plain = getattr(edgegen, builder)(*args, **kw)
    plants = edgegen.planted(builder, k, T, **kw)
    assert set(plants) >= {lab for lab, _, _ in plain}
    mixed = edgegen.iupac(plain, plants)
    letters = np.zeros(256, dtype=bool)
    letters[np.frombuffer(b"RYKMSWBDHVN", dtype=np.uint8)] = True
    for (label, sba, seg), (mlabel, msba, mseg) in zip(plain, mixed):
        assert mlabel == label + "-iupac" and len(msba) == len(sba)
        check_layout(mlabel, msba, mseg, k, acgt_only=False)
        np.testing.assert_array_equal(msba == DOLLAR, sba == DOLLAR, err_msg=label)
        changed = msba != sba
        assert letters[msba[changed]].all() and IS_ACGT[msba[~changed & (msba != DOLLAR)]].all(), label
        copies, keep = plants[label]
        assert copies, label
        for src, dst, n in copies:
            assert n > 0 and src + n <= dst, label
            np.testing.assert_array_equal(sba[dst:dst + n], sba[src:src + n], err_msg=f"{label}: planted {src}->{dst}")
            np.testing.assert_array_equal(msba[dst:dst + n], msba[src:src + n], err_msg=f"{mlabel}: copy {src}->{dst}")
        for lo, hi in keep:
            assert lo < hi and not changed[lo:hi].any(), label
        # about one base in eight outside the kept ranges (binomial: 1/8 +- 5 sigma)
        free = np.ones(len(sba), dtype=bool)
        for lo, hi in keep:
            free[lo:hi] = False
        for src, dst, n in copies:
            free[dst:dst + n] = False
        free &= sba != DOLLAR
        m = int(free.sum())
        assert abs(int(changed[free].sum()) - m / 8) <= 5 * np.sqrt(m * 7 / 64), label
    again = edgegen.iupac(plain, plants)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(mixed, again))


def test_new_builders_are_deterministic():
    for build in (lambda: edgegen.long_ties(5), lambda: edgegen.shared_tails(5),
                  lambda: edgegen.shared_tails(3, edgegen.TAILS_IUPAC)):
        for (la, sa, ga), (lb, sb, gb) in zip(build(), build()):
            assert la == lb and np.array_equal(sa, sb) and np.array_equal(ga, gb)
