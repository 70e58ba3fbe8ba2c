"""Pin tests/lcpref.py (the numpy reference of the LCP array, the spectrum and the position tracks)
before the GPU tests rely on it: against tests/groupref.py -- itself pinned to the golden vectors and
the C oracle -- on all 64 golden cases and every length, and against a per-position dictionary count
on the seq2 cases.  CPU only."""

from collections import Counter

import numpy as np
import pytest

import groupref
import lcpref
from conftest import load_case, load_manifest

CASES = load_manifest()
CASE_IDS = [c["name"] for c in CASES]
NONE_CAP = 12  # the cap of the cases sorted with max_kmer_len None


def cap_of(case):
    return case["max_kmer_len"] or NONE_CAP


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lcp_below_k_is_the_group_head_at_k(case):
    """For every k from 1 to the case's max: lcp < k marks exactly the group heads of group_scan at k,
    distinct[k] is its group count and unique[k] its count of groups of one."""
    a = load_case(case["name"])
    sba, st = a["sba"], a["starts_stable"]
    cap = cap_of(case)
    v = lcpref.lcp(sba, st, cap)
    assert v.dtype == np.uint32 and len(v) == len(st) and v[0] == 0 and v.max() <= cap
    distinct, unique = lcpref.spectrum(v, cap)
    assert distinct[0] == 0 and unique[0] == 0 and len(distinct) == len(unique) == cap + 1
    for k in range(1, cap + 1):
        first, _, _ = groupref.group_scan(sba, st, k, yield_first_n=1)
        heads = np.zeros(len(st), dtype=bool)
        heads[first.astype(np.int64)] = True
        np.testing.assert_array_equal(v < k, heads, err_msg=f"k = {k}")
        hist, total = groupref.group_scan(sba, st, k, max_counts_bin=2)
        assert total == len(st)
        assert distinct[k] == hist.sum() and unique[k] == hist[1], k
        # the array at a smaller cap is the clamped array, and so is its spectrum
        if k in (1, cap // 2, cap - 1):
            np.testing.assert_array_equal(lcpref.lcp(sba, st, k), np.minimum(v, k))
            d_k, u_k = lcpref.spectrum(v, k)
            np.testing.assert_array_equal(d_k, distinct[:k + 1])
            np.testing.assert_array_equal(u_k, unique[:k + 1])


def test_short_kmers_have_lcp_below_their_length_or_at_the_cap():
    """A k-mer cut short after len bases has lcp in [0, len) or equal to cap (two k-mers that end at a
    '$' after the same bases): no per-k-mer length is needed to read groups off the array."""
    seen_cap = 0
    for case in CASES:
        if case["min_kmer_len"] == case["max_kmer_len"]:
            continue
        a = load_case(case["name"])
        sba, st = a["sba"], a["starts_stable"].astype(np.int64)
        cap = cap_of(case)
        v = lcpref.lcp(sba, st, cap).astype(np.int64)
        nd = groupref.bases_before_end(sba)[st]
        short = nd < cap
        assert ((v[short] < nd[short]) | (v[short] == cap)).all(), case["name"]
        seen_cap += int((v[short] == cap).sum())
    assert seen_cap > 0, "some golden case must hold two equal short k-mers"


def _kmer_at(sba, p, k):
    """the bytes that decide equality at length k: up to k bases from p, cut at '$' or the end"""
    w = bytes(sba[p:p + k])
    cut = w.find(b"$")
    return w if cut < 0 else w[:cut]


@pytest.mark.parametrize("case", [c for c in CASES if c["name"].startswith("seq2_min")],
                         ids=[c["name"] for c in CASES if c["name"].startswith("seq2_min")])
def test_tracks_against_a_dictionary_count(case):
    a = load_case(case["name"])
    sba, st = a["sba"], a["starts_stable"].astype(np.int64)
    cap = cap_of(case)
    counts = {k: Counter(_kmer_at(sba, int(p), k) for p in st) for k in range(1, cap + 1)}
    v = lcpref.lcp(sba, st, cap)
    want_unique = np.zeros(len(sba), dtype=np.uint32)
    for p in st.tolist():
        ks = [k for k in range(1, cap + 1) if counts[k][_kmer_at(sba, p, k)] == 1]
        want_unique[p] = ks[0] if ks else lcpref.NEVER_UNIQUE
    np.testing.assert_array_equal(lcpref.min_unique_track(len(sba), st, v, cap), want_unique)
    assert (want_unique[st] >= 1).all()
    if cap <= 2:  # 35 k-mers of at most two bases: some occur twice at every length asked for
        assert (want_unique == lcpref.NEVER_UNIQUE).any()
    if cap >= 6:
        assert ((want_unique > 1) & (want_unique <= cap)).any()
    for k in sorted({1, cap // 2 or 1, cap}):
        want = np.zeros(len(sba), dtype=np.uint32)
        for p in st.tolist():
            want[p] = counts[k][_kmer_at(sba, p, k)]
        np.testing.assert_array_equal(lcpref.multiplicity_track(sba, st, k), want, err_msg=f"k = {k}")
    if case["max_kmer_len"] is None:  # whole k-mers up to '$'
        whole = Counter(_kmer_at(sba, int(p), len(sba)) for p in st)
        want = np.zeros(len(sba), dtype=np.uint32)
        for p in st.tolist():
            want[p] = whole[_kmer_at(sba, p, len(sba))]
        np.testing.assert_array_equal(lcpref.multiplicity_track(sba, st, None), want)
    # positions where no k-mer starts hold 0 in both tracks
    off = np.ones(len(sba), dtype=bool)
    off[st] = False
    assert off.any() and not lcpref.multiplicity_track(sba, st, cap)[off].any()
