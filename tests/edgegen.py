"""Deterministic sort inputs aimed at tile, word and k edges -- TEST INFRASTRUCTURE ONLY (a helper
module, not a conftest).  Numpy only: no GPU, no reference.

gk_sort's position kernels cut the sba into tiles of T positions (24,576 in the L0 count and
partition kernels, 18,432 in the wide L0, 8,192 in the split sort's class-B flag pass, 4,096 in the
key-range select and the encoders) and read a halo of three 32-position groups behind each tile.
Random genomes put a '$', an N run or the end of the array beside a tile edge only by luck; the
builders here put them there on purpose, for a given k and T:

* ``ends``        one contig whose end falls around T and 2T (the last tile holds 0, 1 or 2 k-mers);
* ``separators``  two contigs whose '$' falls around T and 2T, and a contig of exactly k bases laid
                  across T;
* ``comb``        65 contigs of 128 bases: a '$' at every residue mod 64, one stop in every 8-position
                  window, 32-position word and 64-position row;
* ``runs``        mixed-alphabet arrays of about 3 T bases: runs of one non-ACGT letter (none, one,
                  two, 32 and 65 homopolymer k-mers) and single IUPAC letters at T - 1, T, across T,
                  2 T and 3 T, at position 0, at the last byte and on both sides of a '$'.

Every builder returns a list of ``(label, sba, seg_starts)`` with the arrays as SequenceCollection
lays them out (contigs joined by '$', seg_starts the first position of every contig), every contig
holds at least k bases, and every array carries a repeat of 3 k bases twice so that ties occur
beside the edges.  ``runs_plan`` gives the layout ``runs`` builds from; tests/test_edgegen.py pins
the layouts so that a later edit cannot quietly move an edge.
"""

import numpy as np

DOLLAR = 36
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rng(*key):
    return np.random.default_rng([int(x) & 0xFFFFFFFF for x in key])


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].copy()


def _unique(values):
    return list(dict.fromkeys(values))


def segments_of(sba):
    return np.concatenate([[0], np.flatnonzero(np.asarray(sba) == DOLLAR) + 1]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# ends: one contig of L bases
# ---------------------------------------------------------------------------------------------
def end_lengths(k, T):
    """n = L - k + 1 k-mers: L = T + k - 1 and 2 T + k - 1 give exactly T and 2 T; one less and one
    more leave 0 and 2 k-mers beside a full tile; L = T - 1, T, T + 1, 2 T and 2 T + 7 end the array
    (and its halo) around the tile edge; 2 T - k + 1 ends the last k-mer one tile row early."""
    lens = (T - 1, T, T + 1, T + k - 2, T + k - 1, T + k, 2 * T - k + 1, 2 * T, 2 * T + 7, 2 * T + k - 1)
    return [L for L in _unique(lens) if L >= k]


def ends(k, T):
    """The repeat: 3 k bases from T / 4 again as the last 3 k bases (ties among the last k-mers)."""
    out = []
    r = 3 * k
    for L in end_lengths(k, T):
        s = _bases(_rng(1, k, T, L), L)
        s[L - r:L] = s[T // 4:T // 4 + r]
        out.append((f"ends-L{L}", s, np.zeros(1, dtype=np.uint32)))
    return out


# ---------------------------------------------------------------------------------------------
# separators: two contigs
# ---------------------------------------------------------------------------------------------
def separator_offsets(k):
    """'$' at m T + d.  d = 0: the last k-mer of the first contig ends on the last position of a tile;
    d = -1: the first k-mer of the second contig starts on the first position of a tile; d = -k - 1,
    -k, -k + 1: that first k-mer ends on T - 1, T, T + 1; d = k - 1, k: the k-mer that starts on the
    tile's last position (its window is all halo) loses / keeps its last base."""
    return _unique((-k - 1, -k, -k + 1, -1, 0, 1, k - 1, k))


def exact_contig_offsets(k):
    """A contig of exactly k bases at T + o: it ends on T - 1 (o = -k), crosses T by one base from
    either side (o = -k + 1, -1), or starts on T (o = 0)."""
    return _unique((-k, -k + 1, -1, 0))


def separators(k, T, tiles=(1, 2)):
    """The repeat: the 3 k bases before the '$' again behind it (ties on both sides of the '$');
    the exact contig is a copy of the k bases at T / 4 (it ties with that k-mer), the 3 k bases from
    T / 4 are planted again at T / 2."""
    out = []
    r = 3 * k
    for m in tiles:
        for d in separator_offsets(k):
            at = m * T + d
            L = at + 1 + 4 * k + 9
            s = _bases(_rng(2, k, T, m, d), L)
            s[at + 1:at + 1 + r] = s[at - r:at]
            s[at] = DOLLAR
            out.append((f"sep-{m}T{d:+d}", s, np.array([0, at + 1], dtype=np.uint32)))
    for o in exact_contig_offsets(k):
        at = T + o  # the exact contig's first base
        L = at + k
        s = _bases(_rng(3, k, T, o), L)
        s[T // 2:T // 2 + r] = s[T // 4:T // 4 + r]
        s[at:at + k] = s[T // 4:T // 4 + k]
        s[at - 1] = DOLLAR
        out.append((f"exact-T{o:+d}", s, np.array([0, at], dtype=np.uint32)))
    return out


# ---------------------------------------------------------------------------------------------
# comb: a stop every 129 positions
# ---------------------------------------------------------------------------------------------
COMB_CONTIGS, COMB_LEN = 65, 128


def comb(k):
    """'$' at 128, 257, 386, ...: 129 j - 1 = j - 1 (mod 64) for j = 1 .. 64, every residue once.
    The repeat: the first min(3 k, 128) bases of contig 10 again in contig 40."""
    assert k <= COMB_LEN, "every contig needs k bases"
    rng = _rng(4, k)
    contigs = [_bases(rng, COMB_LEN) for _ in range(COMB_CONTIGS)]
    r = min(3 * k, COMB_LEN)
    contigs[40][:r] = contigs[10][:r]
    parts = []
    for c in contigs:
        parts += [c, np.array([DOLLAR], dtype=np.uint8)]
    sba = np.concatenate(parts[:-1])
    return [("comb", sba, segments_of(sba))]


# ---------------------------------------------------------------------------------------------
# tails: the end of the array against a packed word
# ---------------------------------------------------------------------------------------------
def tails(k, B):
    """Single contigs of L = B, B + 1 and B + 31 bases (L = 0, 1, 31 mod 32 for B a multiple of 32:
    no partial last word, one symbol in it, all but one), and two contigs with the '$' on the last and
    the first position of block B.  The repeat: as in ``ends``."""
    out = []
    r = 3 * k
    for L in (B, B + 1, B + 31):
        s = _bases(_rng(5, k, B, L), L)
        s[L - r:L] = s[B // 4:B // 4 + r]
        out.append((f"tail-L{L}", s, np.zeros(1, dtype=np.uint32)))
    for at in (B - 1, B):
        L = at + 1 + 4 * k + 31 - (at + 1 + 4 * k) % 32  # L = 31 mod 32
        s = _bases(_rng(6, k, B, at), L)
        s[at + 1:at + 1 + r] = s[at - r:at]
        s[at] = DOLLAR
        out.append((f"tail-sep{at}", s, np.array([0, at + 1], dtype=np.uint32)))
    return out


# ---------------------------------------------------------------------------------------------
# runs: mixed-alphabet arrays
# ---------------------------------------------------------------------------------------------
RUN_SPLITS = (1, 9, 17, 25, 33)


def run_lengths(k):
    """Runs of one non-ACGT letter with no homopolymer k-mer (k - 1), one (k), two (k + 1), 32
    (32 + k - 1: one whole 32-position group of starts where the run is aligned) and 65 (64 + k: two
    whole groups at any alignment but one)."""
    return [n for n in (k - 1, k, k + 1, 32 + k - 1, 64 + k) if n > 0]


def runs_plan(k, T, lengths=None, splits=None, extras=True):
    """The layouts ``runs`` builds: a list of dicts with ``label``, ``L`` (bytes), ``dollars``
    (positions), ``runs`` [(first, length, letter)] and ``singles`` [(position, letter)].

    Per run length n, two arrays of fixed placements: "fixed-a" has the run at position 0, ending on
    T - 1, starting on 2 T, directly before the '$' and ending on the last byte; "fixed-b" has it
    directly behind the '$', starting on T and ending on 2 T - 1.  Per split s, two arrays whose runs
    straddle T, 2 T and 3 T with s positions before the edge, every run length at one edge (the
    edges rotate with the split; a run no longer than s cannot straddle and is left out).  With
    ``extras``: single IUPAC letters at T - 1, T, T + 31, T + 32 (and around 2 T) and in the last k
    positions of both contigs; R and Y runs (complements: one canonical group); and an array whose
    only non-ACGT byte lies in the last k - 1 positions of its last contig."""
    lengths = run_lengths(k) if lengths is None else list(lengths)
    splits = RUN_SPLITS if splits is None else tuple(splits)
    letters = b"NSWKM"
    plans = []
    for i, n in enumerate(lengths):
        c = letters[i % len(letters)]
        L, d = 3 * T + 11, 2 * T + T // 2
        plans.append(dict(label=f"fixed-a-n{n}", L=L, dollars=[d], singles=[],
                          runs=[(0, n, c), (T - n, n, c), (2 * T, n, c), (d - n, n, c), (L - n, n, c)]))
        L, d = 3 * T + 32, T // 2
        plans.append(dict(label=f"fixed-b-n{n}", L=L, dollars=[d], singles=[],
                          runs=[(d + 1, n, c), (T, n, c), (2 * T - n, n, c)]))
    edges = (T, 2 * T, 3 * T)
    for v, s in enumerate(splits):
        rot = [lengths[(j + v) % len(lengths)] for j in range(len(lengths))]
        for h, part in enumerate((rot[:3], rot[3:])):
            placed = []
            for j, n in enumerate(part):
                E = edges[(j + v + h) % 3]
                if n > s:
                    placed.append((E - s, n, letters[(j + v) % len(letters)]))
            if placed:
                plans.append(dict(label=f"straddle-s{s}-{h}", L=3 * T + T // 4 + 13, dollars=[], singles=[],
                                  runs=sorted(placed)))
    if extras:
        L, d = 3 * T + 5, 2 * T + T // 3
        plans.append(dict(label="letters-a", L=L, dollars=[d], runs=[],
                          singles=[(T - 1, ord("R")), (T + 31, ord("K")), (2 * T + 32, ord("M")), (d - 1, ord("S")),
                                   (L - k, ord("D"))]))
        plans.append(dict(label="letters-b", L=L, dollars=[d], runs=[],
                          singles=[(T, ord("Y")), (T + 32, ord("M")), (2 * T - 1, ord("B")), (2 * T + 31, ord("H")),
                                   (d - k, ord("W")), (L - 1, ord("V"))]))
        n1, n2 = k + 1, 64 + k
        plans.append(dict(label="complement-ry", L=3 * T + 21, dollars=[], singles=[],
                          runs=[(T // 2, n1, ord("R")), (T - 17, n2, ord("R")), (T + T // 2 + 5, n1, ord("Y")),
                                (2 * T - 9, n2, ord("Y")), (2 * T + T // 2, n2, ord("R")),
                                (2 * T + T // 2 + n2 + 40, n1, ord("Y"))]))
        L = 3 * T + 7
        plans.append(dict(label="last-k-only", L=L, dollars=[T + 3], runs=[],
                          singles=[(L - 1 - (k - 1) // 2, ord("N"))]))
    return plans


def runs(k, T, lengths=None, splits=None, extras=True):
    """The repeat: the 3 k bases from T / 4 again at T + T / 4 (clear of every planted letter)."""
    out = []
    r = 3 * k
    for i, p in enumerate(runs_plan(k, T, lengths, splits, extras)):
        s = _bases(_rng(7, k, T, i), p["L"])
        s[T + T // 4:T + T // 4 + r] = s[T // 4:T // 4 + r]
        taken = np.zeros(p["L"], dtype=bool)
        taken[T // 4:T // 4 + r] = taken[T + T // 4:T + T // 4 + r] = True
        for d in p["dollars"]:
            assert not taken[d], (p["label"], d)
            s[d] = DOLLAR
            taken[d] = True
        for a, n, c in p["runs"]:
            lo, hi = max(a - 1, 0), min(a + n + 1, p["L"])
            # a run may touch a '$', nothing else planted
            assert a >= 0 and a + n <= p["L"] and not taken[a:a + n].any(), (p["label"], a)
            assert not (taken[lo:hi] & (s[lo:hi] != DOLLAR)).any(), (p["label"], a)
            s[a:a + n] = c
            taken[a:a + n] = True
        for a, c in p["singles"]:
            assert not taken[a], (p["label"], a)
            s[a] = c
            taken[a] = True
        out.append((p["label"], s, segments_of(s)))
    return out
