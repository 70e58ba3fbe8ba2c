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

The variable-length and suffix-order sorts (min < max, max None; tests/test_gpu_varlen_edges.py)
take ``ends``, ``separators`` and ``comb`` at the tiles of their own kernels -- 4,096 (the position
encoders, the onesweep tile of keys of two or more words, the flag scans), 8,192 (n1 = 8,191 /
8,192 / 8,193 positions: the doubling's rank width changes) and 12,288 (the onesweep tile of
one-word keys) -- and two builders for the prefix-doubling rounds, of about 10-13 k bases each:

* ``long_ties``    a poly-A contig of 6,000 bases between two random contigs, a contig of period 8
                   (ACGTTGCA x 1,000), and a poly-A contig that crosses positions 4,096 and 8,192:
                   groups that stay tied round after round;
* ``shared_tails`` contigs that end in the same n bases, one contig that is exactly those n bases
                   and two contigs that hold them inside, followed by different bases: n = 700, and
                   n around the seed key's symbols (28, 29, 30 for ACGT data; 15, 16, 17 for IUPAC).

``iupac`` turns the arrays of a builder into their IUPAC variant (about one base in eight becomes a
letter of RYKMSWBDHVN; every edge stays where it is), given the builder's ``planted`` copies.

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


# ---------------------------------------------------------------------------------------------
# long_ties: contigs whose suffixes stay tied through the prefix-doubling rounds
# ---------------------------------------------------------------------------------------------
PERIOD8 = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
TIES_REPEAT_AT = 100  # the repeat's offset inside the first and the last (random) contig


def long_ties_plan():
    """[(label, [(kind, bases)])]: the contigs of every array, in order; kind "random", "A" (poly-A)
    or "period8".  The poly-A contig of "polyA-cross" lies on positions 4,001 .. 8,300: it crosses
    4,096 and 8,192."""
    return [("polyA-6000", [("random", 3500), ("A", 6000), ("random", 3500)]),
            ("period8", [("random", 2000), ("period8", 8000), ("random", 2000)]),
            ("polyA-cross", [("random", 4000), ("A", 4300), ("random", 2500)])]


def _ties_repeat(k):
    return min(3 * k, 600)


def _join(contigs):
    parts = []
    for c in contigs:
        parts += [c, np.array([DOLLAR], dtype=np.uint8)]
    sba = np.concatenate(parts[:-1])
    return sba, segments_of(sba)


def long_ties(k):
    """The repeat: min(3 k, 600) bases from offset 100 of the first contig again at offset 100 of the
    last one (both random)."""
    assert k <= 2000, "every contig needs k bases"
    out = []
    r = _ties_repeat(k)
    for i, (label, plan) in enumerate(long_ties_plan()):
        rng = _rng(9, i)
        contigs = []
        for kind, n in plan:
            if kind == "random":
                contigs.append(_bases(rng, n))
            elif kind == "A":
                contigs.append(np.full(n, ord("A"), dtype=np.uint8))
            else:
                contigs.append(np.tile(PERIOD8, n // 8))
        a = TIES_REPEAT_AT
        contigs[-1][a:a + r] = contigs[0][a:a + r]
        sba, seg = _join(contigs)
        out.append((label, sba, seg))
    return out


# ---------------------------------------------------------------------------------------------
# shared_tails: equal '$'-terminated tails, which no doubling round can separate
# ---------------------------------------------------------------------------------------------
TAILS_ACGT = (700, 28, 29, 30)   # 29: the symbols of the ACGT seed key
TAILS_IUPAC = (700, 15, 16, 17)  # 16: the symbols of the IUPAC seed key


def shared_tails_plan(k, tails=TAILS_ACGT):
    """[dict(label, n, contigs)]: per tail length n the contigs as (bases, offset of the tail or
    None), in order -- "end" contigs of 2,000, 2,500 and 1,800 bases that end in the tail, the
    "exact" contig that is the tail alone (left out where n < k), two "inside" contigs of 800 random
    bases, the tail, one base ('T' in the first, 'C' in the second: the second sorts first although
    it lies behind) and 799 more random bases, and a random contig of 600 bases.  The first contig
    ends in the tail, so the tail's lowest position has exactly n bases up to its '$'."""
    plans = []
    for n in tails:
        contigs = [(2000, 2000 - n)]
        if n >= k:
            contigs.append((n, 0))
        contigs += [(800 + n + 800, 800), (800 + n + 800, 800), (2500, 2500 - n), (1800, 1800 - n), (600, None)]
        plans.append(dict(label=f"tail{n}", n=n, contigs=contigs, before=None))
    # "lone": one end contig and the two inside contigs, the bases before their tails 'A', 'C', 'G' --
    # no two suffixes that begin one base before a tail tie, so with n the seed key's symbols the
    # tails are the only group still tied after the seed sort, and no round repairs what the check
    # for finished groups lets through; two random contigs fill the array up
    for n in tails[1:]:
        contigs = [(2000, 2000 - n), (800 + n + 800, 800), (800 + n + 800, 800), (4500, None), (600, None)]
        plans.append(dict(label=f"tail{n}-lone", n=n, contigs=contigs, before="ACG"))
    return plans


def shared_tails(k, tails=TAILS_ACGT):
    """The repeat: the tails themselves."""
    assert k <= 600, "every contig needs k bases"
    out = []
    for p in shared_tails_plan(k, tails):
        n = p["n"]
        rng = _rng(10, n) if p["before"] is None else _rng(10, n, 1)
        tail = _bases(rng, n)
        contigs, inside, holder = [], 0, 0
        for length, at in p["contigs"]:
            c = _bases(rng, length)
            if at is not None:
                c[at:at + n] = tail
                if p["before"]:
                    c[at - 1] = ord(p["before"][holder])
                holder += 1
                if at + n < length:  # an "inside" contig: the base behind the tail
                    c[at + n] = ord("TC"[inside])
                    inside += 1
            contigs.append(c)
        sba, seg = _join(contigs)
        out.append((p["label"], sba, seg))
    return out


def tail_positions(k, tails=TAILS_ACGT):
    """label -> [the tail's first position in every contig that holds it], ascending"""
    out = {}
    for p in shared_tails_plan(k, tails):
        pos, first = [], 0
        for length, at in p["contigs"]:
            if at is not None:
                pos.append(first + at)
            first += length + 1
        out[p["label"]] = pos
    return out


# ---------------------------------------------------------------------------------------------
# the IUPAC variant of a builder's arrays
# ---------------------------------------------------------------------------------------------
IUPAC_LETTERS = np.frombuffer(b"RYKMSWBDHVN", dtype=np.uint8)


def planted(builder, k, T=None, tails=TAILS_ACGT, tiles=(1, 2)):
    """label -> (copies, keep) of the arrays of ``builder(k, T)`` (``tiles``, ``tails``: as given to
    ``separators`` / ``shared_tails``): copies [(source, destination,
    bases)] are the planted repeats in the order the builder writes them, keep [(first, one past
    the last)] the ranges whose bases make the array what it is (tied contigs, the base behind an
    inside tail)."""
    r = 3 * k
    out = {}
    if builder == "ends":
        for L in end_lengths(k, T):
            out[f"ends-L{L}"] = ([(T // 4, L - r, r)], [])
    elif builder == "separators":
        for m in tiles:
            for d in separator_offsets(k):
                at = m * T + d
                out[f"sep-{m}T{d:+d}"] = ([(at - r, at + 1, r)], [])
        for o in exact_contig_offsets(k):
            out[f"exact-T{o:+d}"] = ([(T // 4, T // 2, r), (T // 4, T + o, k)], [])
    elif builder == "comb":
        out["comb"] = ([(10 * (COMB_LEN + 1), 40 * (COMB_LEN + 1), min(r, COMB_LEN))], [])
    elif builder == "long_ties":
        for label, plan in long_ties_plan():
            first = [0]
            for _, n in plan:
                first.append(first[-1] + n + 1)
            a = TIES_REPEAT_AT
            keep = [(first[i], first[i] + n) for i, (kind, n) in enumerate(plan) if kind != "random"]
            out[label] = ([(a, first[len(plan) - 1] + a, _ties_repeat(k))], keep)
    elif builder == "shared_tails":
        plans = {p["label"]: p for p in shared_tails_plan(k, tails)}
        for label, pos in tail_positions(k, tails).items():
            n = plans[label]["n"]
            holders = [(length, at) for length, at in plans[label]["contigs"] if at is not None]
            keep = [(q + n, q + n + 1) for q, (length, at) in zip(pos, holders) if at + n < length]
            if plans[label]["before"]:
                keep += [(q - 1, q) for q in pos]
            out[label] = ([(pos[0], q, n) for q in pos[1:]], keep)
    else:
        raise ValueError(builder)
    return out


def iupac(arrays, plants, share=8):
    """The arrays with one base in ``share`` (seeded per array) turned into a letter of RYKMSWBDHVN:
    no '$' and no kept range is touched, and the planted copies are written again from their
    sources, so every copy still equals its source and every edge lies where it lay."""
    out = []
    for i, (label, sba, seg) in enumerate(arrays):
        copies, keep = plants[label]
        s = sba.copy()
        rng = _rng(8, i, len(s))
        hit = (rng.integers(0, share, len(s)) == 0) & (s != DOLLAR)
        for lo, hi in keep:
            hit[lo:hi] = False
        assert hit.any(), label
        s[hit] = IUPAC_LETTERS[rng.integers(0, len(IUPAC_LETTERS), int(hit.sum()))]
        for src, dst, n in copies:
            s[dst:dst + n] = s[src:src + n]
        assert (s[sba == DOLLAR] == DOLLAR).all() and ((s == DOLLAR) == (sba == DOLLAR)).all(), label
        out.append((label + "-iupac", s, seg))
    return out
