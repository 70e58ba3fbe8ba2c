"""tests/screenref.py (the numpy reference of the read screen) pinned against a pure-Python brute force
-- a dict of the genome's substrings -- on small inputs.  No GPU, no library."""

import numpy as np
import pytest

import screenref

COMPLEMENT = dict(screenref.COMPLEMENT)


def rc(s: str) -> str:
    return "".join(COMPLEMENT[ch] for ch in reversed(s))


def brute(contigs, K, reads, canonical=False, both_strands=False):
    table = {}
    for contig in contigs:
        for i in range(len(contig) - K + 1):
            w = contig[i:i + K]
            if canonical:
                w = min(w, rc(w))
            table[w] = table.get(w, 0) + 1
    wc, n_windows, n_present, occ = [], [], [], []
    for read in reads:
        counts = []
        for i in range(len(read)):
            c = 0
            if i + K <= len(read):
                w = read[i:i + K]
                if canonical:
                    c = table.get(min(w, rc(w)), 0)
                else:
                    c = table.get(w, 0)
                    if both_strands and rc(w) != w:
                        c += table.get(rc(w), 0)
            counts.append(c)
        wc += counts
        n_windows.append(max(0, len(read) - K + 1))
        n_present.append(sum(1 for c in counts if c > 0))
        occ.append(sum(counts))
    return wc, n_windows, n_present, occ


def check(contigs, K, reads, canonical=False, both_strands=False):
    sba = screenref.as_sba([(f"c{i}", c) for i, c in enumerate(contigs)])
    ref = screenref.screen(sba, K, reads, canonical, both_strands)
    wc, n_windows, n_present, occ = brute(contigs, K, reads, canonical, both_strands)
    assert ref["window_counts"].dtype == np.uint32 and ref["n_windows"].dtype == np.uint32
    assert ref["n_present"].dtype == np.uint32 and ref["occurrences"].dtype == np.uint64
    assert ref["window_counts"].tolist() == wc
    assert ref["n_windows"].tolist() == n_windows
    assert ref["n_present"].tolist() == n_present
    assert ref["occurrences"].tolist() == occ
    assert ref["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in reads])]).tolist()
    return ref


def rand(seed, n, letters="ACGT"):
    rng = np.random.default_rng(seed)
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


GENOME = [rand(1, 300) + "AAAAAAAAAAAA" + rand(2, 200), rand(3, 150)]
MIXED = [rand(4, 120) + "NNNNNNNN" + rand(5, 80, "ACGTRYKMSWN"), "ACGTNRY" * 9]


@pytest.mark.parametrize("K", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("canonical,both", [(False, False), (False, True), (True, False), (True, True)])
def test_against_brute_force(K, canonical, both):
    g = GENOME[0]
    reads = [g[10:60], "", g[100:100 + K], g[200:200 + K + 1], g[50:50 + K - 1], rc(g[300:340]), rand(9, 40),
             "A" * 20, "ACGT" * 4, "N" * 9, g[290:330] + "N" + g[331:350], "", "T" * (K + 2), g[-K:]]
    ref = check(GENOME, K, reads, canonical, both)
    assert screenref.nontrivial(ref)


@pytest.mark.parametrize("K", [3, 6])
@pytest.mark.parametrize("canonical,both", [(False, False), (False, True), (True, False)])
def test_mixed_genome_and_iupac_reads(K, canonical, both):
    m = MIXED[0]
    reads = [m[100:150], m[115:135], "NNNNNNNNNN", "ACGTNRYACGTNRY", rc(m[110:140]), "RYKMSW" * 3, "", "N"]
    ref = check(MIXED, K, reads, canonical, both)
    assert (ref["window_counts"] > 0).any()


def test_palindromes_at_even_k_count_once():
    # ACGT and AATT are their own reverse complements
    contigs = ["ACGTACGTTTAATTAA"]
    reads = ["ACGT", "AATT", "ACGTAATT"]
    plain = check(contigs, 4, reads)
    both = check(contigs, 4, reads, both_strands=True)
    canon = check(contigs, 4, reads, canonical=True)
    assert plain["window_counts"][0] == 2 and both["window_counts"][0] == 2 and canon["window_counts"][0] == 2
    assert plain["window_counts"][4] == 1 and both["window_counts"][4] == 1


def test_reads_around_k_and_empty_batches():
    contigs = ["ACGTTGCA"]
    for K in (3, 4):
        ref = check(contigs, K, ["", "AC", "ACGTTGCA"[:K - 1], "ACGTTGCA"[:K], "ACGTTGCA"[:K + 1], ""])
        assert ref["n_windows"].tolist() == [0, 0, 0, 1, 2, 0]
    ref = check(contigs, 3, [])
    assert len(ref["window_counts"]) == 0 and len(ref["n_present"]) == 0
    ref = check(contigs, 3, ["", ""])
    assert ref["occurrences"].tolist() == [0, 0]
    ref = check(contigs, 9, ["ACGTTGCA"])  # K above the genome's and the read's length
    assert ref["n_windows"].tolist() == [0]


@pytest.mark.parametrize("K", [2, 4, 5, 7])
def test_both_strands_forward_equals_plain_canonical(K):
    g = GENOME[0]
    reads = [g[20:90], rc(g[150:230]), rand(11, 60), "ACGT" * 5, "", "A" * 15, MIXED[0][100:140]]
    for contigs in (GENOME, MIXED):
        sba = screenref.as_sba([(f"c{i}", c) for i, c in enumerate(contigs)])
        both = screenref.screen(sba, K, reads, canonical=False, both_strands=True)
        canon = screenref.screen(sba, K, reads, canonical=True)
        for name in ("window_counts", "n_windows", "n_present", "occurrences"):
            np.testing.assert_array_equal(both[name], canon[name], err_msg=name)
        flagged = screenref.screen(sba, K, reads, canonical=True, both_strands=True)  # the flag changes nothing
        np.testing.assert_array_equal(flagged["window_counts"], canon["window_counts"])


def test_window_never_spans_two_reads_or_two_contigs():
    contigs = ["AAAC", "GTTT"]
    ref = check(contigs, 4, ["AAAC", "GTTT", "AAACGTTT", "AA", "ACGT"])
    assert ref["window_counts"].tolist()[:8] == [1, 0, 0, 0, 1, 0, 0, 0]
    assert ref["n_present"].tolist() == [1, 1, 2, 0, 0]  # ACGT spans the contigs: absent
    joined = check(contigs, 2, ["AC", "CG", "A", "C"])   # C|G spans the contigs; A + C are two reads
    assert joined["n_present"].tolist() == [1, 0, 0, 0]
