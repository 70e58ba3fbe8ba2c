"""The NumPy reference of gk_minimizers (tests/minimizerref.py) against itself, no GPU: the definition by
windows, the local rule and a pure-Python loop agree; the order hash equals its big-integer form."""

import numpy as np
import pytest

import minimizerref as ref
from genome_kmers.kmers import MinimizerResult  # noqa: F401  (the feature under test)

KS = (1, 2, 3, 16, 31, 32)
WS = (1, 2, 3, 10, 64)


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def inputs():
    rng = np.random.default_rng(11)
    rnd = random_bases(rng, 420)
    interrupted = bytearray(random_bases(rng, 400))
    for p in (0, 57, 58, 130, 250, 251, 252, 399):
        interrupted[p] = ord("N")
    interrupted[300] = ord("$")
    interrupted[310] = ord("R")
    multi = [random_bases(rng, n) for n in (90, 0, 31, 32, 33, 1, 0, 140, 5, 70)]
    return {
        "random": [rnd],
        "polyA": [b"A" * 300],
        "period2": [b"AC" * 150],
        "period3": [b"ACG" * 100 + b"T" + b"GCA" * 40],
        "interrupted": [bytes(interrupted)],
        "multi": multi,
    }


INPUTS = inputs()


def python_loop(seqs, k, w, canonical, lex):
    """The definition in plain Python, one sequence and one window at a time."""
    pos, keys, strands, per_seq = [], [], [], []
    base = 0
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    for s in seqs:
        info = []  # per position: None, or (ord, ckey, strand)
        for p in range(len(s)):
            kmer = s[p:p + k]
            if len(kmer) < k or any(b not in code for b in kmer):
                info.append(None)
                continue
            key = 0
            for b in kmer:
                key = (key << 2) | code[b]
            rc = ref.revcomp_key(key, k)
            ckey, strand = (rc, 1) if canonical and rc < key else (key, 0)
            info.append((ckey if lex else ref.mix(ckey), ckey, strand))
        chosen = set()
        for a in range(len(s) - w + 1):
            win = info[a:a + w]
            if any(x is None for x in win):
                continue
            best = min(range(w), key=lambda i: (win[i][0], i))
            chosen.add(a + best)
        for p in sorted(chosen):
            pos.append(base + p)
            keys.append(info[p][1])
            strands.append(info[p][2])
        per_seq.append(len(chosen))
        base += len(s)
    return (np.array(pos, dtype=np.uint64), np.array(keys, dtype=np.uint64), np.array(strands, dtype=np.uint8),
            np.array(per_seq, dtype=np.uint32))


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_three_implementations_agree(name, k):
    seqs = INPUTS[name]
    arr, off = ref.as_batch(seqs)
    nontrivial = 0
    for w in WS:
        for lex in (False, True):
            for canonical in (False, True):
                a = ref.by_windows(arr, off, k, w, canonical, lex)
                b = ref.by_local_rule(arr, off, k, w, canonical, lex)
                c = python_loop(seqs, k, w, canonical, lex)
                assert same(a, b) and same(a, c), (name, k, w, lex, canonical)
                assert int(a[3].sum()) == a[0].size
                nvalid = int(ref.position_keys(arr, off, k, canonical)[0].sum())
                nontrivial += 0 < a[0].size < nvalid
                if w == 1:
                    assert a[0].size == nvalid
    if name == "random":
        assert nontrivial > 0


def test_mix_fixed_values():
    # computed here with Python big integers, step by step
    def slow(x):
        h = x ^ 0x9E3779B97F4A7C15
        for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
            h ^= h >> 33
            h = (h * mul) % (1 << 64)
        return h ^ (h >> 33)

    for x in (0, 1, (1 << 64) - 1):
        assert ref.mix(x) == slow(x)
        assert int(ref.mix_np(np.array([x], dtype=np.uint64))[0]) == slow(x)
    assert (ref.mix(0), ref.mix(1), ref.mix((1 << 64) - 1)) == (0x9CA066F1A4AB2EEA, 0x25B775FAECA8F520,
                                                                 0x3CD617BBBCC39640)  # (the driver pins the same)
    assert ref.mix(0) != 0  # (poly-A does not hash to the least ord)
    assert ref.mix(0) == ref.fmix64(0x9E3779B97F4A7C15)


def test_mix_is_injective_on_a_sample():
    rng = np.random.default_rng(5)
    x = np.unique(np.concatenate([rng.integers(0, 1 << 63, 100_000, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                                  np.arange(1000, dtype=np.uint64)]))
    assert np.unique(ref.mix_np(x)).size == x.size


def test_no_window_across_reads_at_k1():
    # two reads of 3 bases: at k = 1, w = 4 the six valid starts are consecutive bytes, yet no window exists
    arr, off = ref.as_batch([b"ACG", b"TAC"])
    for fn in (ref.by_windows, ref.by_local_rule):
        pos, _, _, per_seq = fn(arr, off, 1, 4)
        assert pos.size == 0 and per_seq.tolist() == [0, 0]
        pos, _, _, per_seq = fn(arr, off, 1, 3, lex=True)  # one window per read: A of the first, A of the second
        assert pos.tolist() == [0, 4] and per_seq.tolist() == [1, 1]
    one, off1 = ref.as_batch([b"ACGTAC"])
    assert ref.by_windows(one, off1, 1, 4, lex=True)[0].tolist() == [0, 4]


def test_canonical_key_and_strand():
    arr, off = ref.as_batch([b"ACGT", b"TTTT", b"AAAC"])
    _, ckey, strand, _ = ref.by_windows(arr, off, 4, 1, canonical=True, lex=True)
    # ACGT is its own reverse complement (strand 0); TTTT -> AAAA (strand 1); AAAC < GTTT (strand 0)
    assert ckey.tolist() == [0b00011011, 0, 1] and strand.tolist() == [0, 1, 0]
    assert ref.revcomp_key(0b00011011, 4) == 0b00011011 and ref.revcomp_key((1 << 64) - 1, 32) == 0


def test_density_on_random_bases():
    rng = np.random.default_rng(3)
    arr, off = ref.as_batch([random_bases(rng, 100_000)])
    pos = ref.by_local_rule(arr, off, 15, 10)[0]
    density = pos.size / (100_000 - 14)
    assert 1 / 10 < density < 1  # (about 2 / (w + 1) for a random order)
    assert np.all(np.diff(pos.astype(np.int64)) <= 10)  # consecutive minimizers are at most w apart
