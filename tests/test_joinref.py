"""tests/joinref.py, the host reference of the two-genome join, pinned on cases written out by hand
and against gk_lookup's documented convention (first = the number of sorted k-mers that compare less,
count = the number that match) through the oracle's sorted starts of a golden case.  No GPU."""

from bisect import bisect_left, bisect_right

import numpy as np

import joinref
from conftest import load_case, load_manifest


def S(*kmers):
    return [k.encode() for k in kmers]


def test_windows_do_not_span_a_contig_end():
    # two contigs: ACGT and GTA; the windows CG T$G, T$GT ... hold '$' and are no k-mers
    rows = joinref.kmer_rows([("c0", "ACGT"), ("c1", "GTA")], 3)
    assert rows.tolist() == S("ACG", "CGT", "GTA")
    assert joinref.kmer_rows([("c0", "ACGT"), ("c1", "GT")], 3).tolist() == S("ACG", "CGT")
    assert joinref.kmer_rows("AC", 3).tolist() == []
    assert joinref.as_sba([("c0", "ACGT"), ("c1", "GTA")]).tobytes() == b"ACGT$GTA"


def test_duplicates_and_insertion_points():
    # A: AAC ACA CAA AAC ACG  -> distinct AAC x2, ACA, ACG, CAA
    # B: ACA CAT ATA TAC ACA CAA (ACATACAA) -> sorted: ACA ACA ATA CAA CAT TAC
    r = joinref.join("AACAACG", "ACATACAA", 3)
    assert r["a_kmers"].tolist() == S("AAC", "ACA", "ACG", "CAA")
    assert r["a_count"].tolist() == [2, 1, 1, 1]
    assert r["b_kmers"].tolist() == S("ACA", "ATA", "CAA", "CAT", "TAC")
    assert r["b_mult"].tolist() == [2, 1, 1, 1, 1]
    # AAC: below everything (0); ACA: first 0, twice; ACG: after the two ACA (2), absent; CAA: after ATA (3)
    assert r["b_first"].tolist() == [0, 0, 2, 3] and r["b_first"].dtype == np.uint64
    assert r["b_count"].tolist() == [0, 2, 0, 1] and r["b_count"].dtype == np.uint32
    assert r["stats"] == {"n_distinct_a": 4, "n_distinct_b": 5, "n_shared": 2, "occ_a_shared": 2, "occ_b_shared": 3,
                          "occ_min": 2}
    d = joinref.derived(r["stats"])
    assert d["jaccard"] == 2 / 7 and d["containment"] == 2 / 4
    # a k-mer above all of B: its insertion point is B's k-mer count
    r = joinref.join("TTT", "ACATACAA", 3)
    assert r["b_first"].tolist() == [6] and r["b_count"].tolist() == [0]


def test_identity_and_empty_sides():
    r = joinref.join("AACAACG", "AACAACG", 3)
    np.testing.assert_array_equal(r["b_count"], r["a_count"])
    assert r["b_first"].tolist() == [0, 2, 3, 4]  # the group starts of AAC AAC ACA ACG CAA
    assert r["stats"]["n_shared"] == 4 and r["stats"]["occ_min"] == 5
    assert joinref.derived(r["stats"]) == {"jaccard": 1.0, "containment": 1.0}
    e = joinref.join("AC", "AACAACG", 3)
    assert e["stats"] == dict.fromkeys(joinref.STAT_NAMES, 0) | {"n_distinct_b": 4}
    assert len(e["b_first"]) == 0
    e = joinref.join("AACAACG", "AC", 3)
    assert e["b_first"].tolist() == [0, 0, 0, 0] and e["b_count"].tolist() == [0, 0, 0, 0]
    assert joinref.derived(joinref.join("AC", "AC", 3)["stats"]) == {"jaccard": 0.0, "containment": 0.0}


def test_canonical_forms_and_a_palindrome():
    # ACGT is its own reverse complement; AAAC <-> GTTT: canonical AAAC; with an IUPAC letter: ARTC -> GAYT
    rows = joinref.kmer_rows([("c0", "ACGT"), ("c1", "GTTT"), ("c2", "GAYT")], 4, canonical=True)
    assert rows.tolist() == S("ACGT", "AAAC", "ARTC")
    # A holds GTTT, B holds AAAC and the palindrome on both: all shared under canonical, not forward
    a, b = [("c0", "GTTT"), ("c1", "ACGT")], [("c0", "AAAC"), ("c1", "ACGT"), ("c2", "ACGT")]
    r = joinref.join(a, b, 4, canonical=True)
    assert r["a_kmers"].tolist() == S("AAAC", "ACGT")
    assert r["b_count"].tolist() == [1, 2] and r["b_first"].tolist() == [0, 1]
    f = joinref.join(a, b, 4)
    assert f["a_kmers"].tolist() == S("ACGT", "GTTT") and f["b_count"].tolist() == [2, 0]
    assert f["b_first"].tolist() == [1, 3]
    # W, S, N are their own complements: an odd palindrome
    assert joinref.kmer_rows("ACWGT", 5, canonical=True).tolist() == S("ACWGT")
    assert joinref.COMP[np.frombuffer(b"ACGTRYKMBVDHSWN$", dtype=np.uint8)].tobytes() == b"TGCAYRMKVBHDSWN$"


def test_against_the_lookup_convention_on_golden_cases():
    """gk_lookup documents: first = the sorted k-mers that compare less, count = those that match, with
    a k-mer cut at its contig's end below its extensions.  Over the oracle's sorted starts
    (``starts_stable``) of a fixed-length golden case that is a bisect; joinref gives the same."""
    cases = {c["name"]: c for c in load_manifest()}
    for name_a, name_b in (("rand10k_k31", "rand10k_k31"), ("repeat_k31", "rand10k_k31"),
                           ("iupac_k31", "repeat_k31")):
        K = cases[name_b]["max_kmer_len"]
        assert cases[name_b]["min_kmer_len"] == K == cases[name_a]["max_kmer_len"]
        a, b = load_case(name_a), load_case(name_b)
        raw = bytes(b["sba"])
        t = [raw[s:s + K].split(b"$")[0] for s in b["starts_stable"].tolist()]
        assert t == sorted(t) and all(len(x) == K for x in t)
        r = joinref.join(a["sba"], b["sba"], K)
        assert len(r["a_kmers"]) > 0
        queries = r["a_kmers"].tolist()
        first = [bisect_left(t, q) for q in queries]
        count = [bisect_right(t, q) - f for q, f in zip(queries, first)]
        assert r["b_first"].tolist() == first
        assert r["b_count"].tolist() == count
