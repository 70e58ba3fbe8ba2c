"""Pin tests/groupref.py (the numpy reference of the group scan) before the GPU tests rely on it:
against the golden vectors the reference itself produced, and against the C oracle (gk_oracle.c)
for every built-in filter kind and every parameter edge tests/test_gpu_groups.py uses.  CPU only.
"""

import ctypes

import numpy as np
import pytest

import groupref
from conftest import load_case, load_manifest
from genome_kmers import kmers as gk
from oracle import oracle
from test_gpu_parity import FILTER_SPECS, filter_of, random_genome

CASES = load_manifest()
CASE_IDS = [c["name"] for c in CASES]


# ---------------------------------------------------------------------------------------------
# golden vectors
# ---------------------------------------------------------------------------------------------
def _golden_query(sba, starts, q):
    filt = oracle.filter_params(q["filter"])
    kw = dict(min_group_size=q["min_group_size"], max_group_size=q["max_group_size"])
    if q["op"] == "group_counts":
        kw["max_counts_bin"] = q["max_counts_bin"]
    elif q["op"] == "count":
        kw["max_counts_bin"] = 1000000
    else:
        kw["yield_first_n"] = q.get("yield_first_n")
    res = groupref.scan_filtered(sba, starts, q["kmer_len"], filt, **kw)
    if res[0] == "raise":
        exc = gk._filter_error(res[2], res[1], filter_of(q["filter"]))
        return {"error": type(exc).__name__, "message": str(exc)}
    if q["op"] == "group_counts":
        return {"hist": res[1][0].tolist(), "total": res[1][1]}
    if q["op"] == "count":
        return {"total": res[1][1]}
    return {"kmers": [list(t) for t in zip(*(a.tolist() for a in res[1]))]}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_golden_queries_match_reference(case):
    """Every golden query with the minimum k-mer info, on the reference's break_ties=True order:
    histograms, totals, yields, and the exception type and message of a raising filter."""
    a = load_case(case["name"])
    checked = 0
    for q, want in zip(case["queries"], case["results_stable_order"]):
        if q.get("info", "minimum") != "minimum":
            continue
        assert _golden_query(a["sba"], a["starts_stable"], q) == want, q
        checked += 1
    assert checked > 0


def test_golden_set_has_raising_filters_and_yields():
    kinds = {(q["op"], "error" in r) for c in CASES for q, r in zip(c["queries"], c["results_stable_order"])}
    assert {("count", True), ("count", False), ("get_kmers", False), ("group_counts", False)} <= kinds


# ---------------------------------------------------------------------------------------------
# the C oracle, filter by filter
# ---------------------------------------------------------------------------------------------
def _oracle_scan(sba, st, kmer_len, filt, is_sorted, **kw):
    try:
        return "ok", oracle.group_scan(sba, st, kmer_len, filt, is_sorted=is_sorted, **kw)
    except oracle.OracleError as e:
        return "raise", e.idx, e.kind


def _ref_scan(sba, st, kmer_len, evaluated, is_sorted, **kw):
    """the reference's answer in the oracle's shapes; evaluated = filter_eval's (passes, err_code)"""
    passes, err = evaluated
    raised = groupref.first_raise(st, err)
    if raised is not None:
        return "raise", raised[0], groupref.ORACLE_ERROR_KIND[raised[1]]
    res = groupref.group_scan(sba, st, kmer_len, valid=passes, is_sorted=is_sorted, **kw)
    if "max_counts_bin" in kw:
        return "ok", (res[0].tolist(), res[1])
    return "ok", list(zip(*(a.tolist() for a in res)))


SELECTIONS = [dict(max_counts_bin=100), dict(max_counts_bin=3, min_group_size=2, max_group_size=5),
              dict(min_group_size=2, yield_first_n=2), dict(), dict(max_group_size=3, yield_first_n=1)]
# for 126 k k-mers: no selection that yields nearly every k-mer as a Python tuple
FEW_YIELDS = SELECTIONS[:3] + [dict(min_group_size=2, max_group_size=3, yield_first_n=1)]


def _check_vs_oracle(sba, st, kmer_lens, filters, selections=SELECTIONS):
    """-> the set of (label, outcome) seen, for the callers' premise asserts"""
    seen = set()
    for label, filt in filters:
        evaluated = groupref.filter_eval(sba, st, *filt)
        for kmer_len in kmer_lens:
            for is_sorted in (True, False) if kmer_len == kmer_lens[0] else (True,):
                for kw in selections:
                    want = _oracle_scan(sba, st, kmer_len, filt, is_sorted, **kw)
                    if want[0] == "ok" and "max_counts_bin" in kw:
                        want = ("ok", (want[1][0].tolist(), want[1][1]))
                    got = _ref_scan(sba, st, kmer_len, evaluated, is_sorted, **kw)
                    assert got == want, (label, kmer_len, is_sorted, kw)
                seen.add((label, want[0]))
    return seen


def _builtin_filter_sequence():
    """The sequence of test_builtin_filters_per_position_vs_oracle (tests/test_gpu_parity.py): IUPAC
    letters, N runs, three ragged contigs."""
    rng = np.random.default_rng(21)
    rep = rng.choice(np.frombuffer(b"ACGTACGTGCCGGS", dtype=np.uint8), 900).astype(np.uint8)
    seqs = random_genome(rng, [60_000, 41_003, 25_017], alphabet=b"ACGTACGTACGTACGTNRY", repeat=rep, copies=6)
    seqs = [s[:5000] + "N" * 700 + s[5000:] for _, s in seqs]
    return np.frombuffer("$".join(seqs).encode(), dtype=np.uint8)


def test_iupac_contigs_every_filter_vs_oracle():
    sba = _builtin_filter_sequence()
    unsorted = groupref.enumerate_starts(sba, 31)
    np.testing.assert_array_equal(unsorted, oracle.enumerate_starts(sba, groupref.segments_of(sba), 31))
    st = oracle.quicksort(sba, unsorted, 31, 31, break_ties=True)
    filters = [("-".join(str(v) for v in s.values()), oracle.filter_params(s)) for s in FILTER_SPECS]
    filters += groupref.filter_cases(31) + [("keep-all", (0, 0, 0, 0))]
    seen = _check_vs_oracle(sba, st, [16, 31, 40], filters, FEW_YIELDS)  # below, at and above the sort length
    for kind in ("homopolymer", "gc", "no-ambiguous"):
        assert (f"{kind}-raises", "raise") in seen
    assert sum(1 for _, outcome in seen if outcome == "ok") >= 15


def test_acgt_repeats_every_filter_vs_oracle():
    rng = np.random.default_rng(5)
    rep = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 700).astype(np.uint8)
    seqs = random_genome(rng, [14_000, 6_001], repeat=rep, copies=5)
    sba = np.frombuffer("$".join(s for _, s in seqs).encode(), dtype=np.uint8)
    st = oracle.quicksort(sba, groupref.enumerate_starts(sba, 20), 20, 20, break_ties=True)
    hist, _ = groupref.group_scan(sba, st, 20, max_counts_bin=8)
    assert hist[2:].sum() > 500, "the planted repeats must give groups"
    _check_vs_oracle(sba, st, [8, 20, 25, None], groupref.filter_cases(20) + [("keep-all", (0, 0, 0, 0))])


@pytest.mark.parametrize("sba_len,contigs,K,n_run", groupref.EDGE_INPUTS,
                         ids=[f"sba{e[0]}-k{e[2]}" for e in groupref.EDGE_INPUTS])
def test_filter_edge_inputs_vs_oracle(sba_len, contigs, K, n_run):
    """The inputs and parameters of the device's filter-edge tests: every case of filter_cases(K) on
    the sorted and the unsorted starts, and the CRISPR start set that reads across '$'."""
    sba = groupref.iupac_sequence(sba_len, contigs, seed=sba_len, n_run=n_run)
    unsorted = groupref.enumerate_starts(sba, K)
    st = oracle.quicksort(sba, unsorted, K, K, break_ties=True)
    _check_vs_oracle(sba, st, [K], groupref.filter_cases(K))
    _check_vs_oracle(sba, unsorted, [K], groupref.filter_cases(K))
    inner = groupref.crispr_safe_starts(sba, st)
    seen = _check_vs_oracle(sba, inner, [K], [("crispr-ngg", (groupref.CRISPR_NGG, 0, 0, 0))])
    assert seen == {("crispr-ngg", "ok")}


@pytest.mark.parametrize("sba_len,contigs,K,n_run", groupref.EDGE_INPUTS,
                         ids=[f"sba{e[0]}-k{e[2]}" for e in groupref.EDGE_INPUTS])
def test_filter_eval_every_position_vs_oracle(sba_len, contigs, K, n_run):
    """filter_eval at EVERY base of the sba (k-mers of one base included), one gko_filter call per
    start: pass / fail / raise code of each k-mer, so the precedence inside a k-mer is pinned for
    windows that meet a '$' or the end at every offset."""
    sba = groupref.iupac_sequence(sba_len, contigs, seed=sba_len, n_run=n_run)
    starts = groupref.enumerate_starts(sba, 1)
    code_of = {-10: 1, -11: 2, -12: 3, -13: 4, -14: 5, -15: 6}
    ptr = sba.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    f = oracle.lib().gko_filter
    outcomes = set()
    for label, (kind, p0, p1, p2) in groupref.filter_cases(K):
        passes, err = groupref.filter_eval(sba, starts, kind, p0, p1, p2)
        want = np.array([f(ptr, len(sba), kind, p0, p1, p2, int(s)) for s in starts])
        np.testing.assert_array_equal(passes, want == 1, err_msg=label)
        np.testing.assert_array_equal(err, [code_of.get(int(w), 0) for w in want], err_msg=label)
        outcomes.update(np.unique(err).tolist())
    # every gk_filter_error code occurs; the two that need a '$' only where the sba has one
    assert outcomes == ({0, 1, 2, 3, 4, 5, 6} if contigs else {0, 1, 3, 4, 6})


def test_group_scan_head_masks():
    """heads= (GK_GROUPS_FROM_HEADS): heads count at valid positions only, the first valid k-mer
    starts a group whatever its head says; is_sorted=False: one group per valid k-mer."""
    sba = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    st = np.arange(8, dtype=np.uint32)
    valid = np.array([0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)
    heads = np.array([1, 0, 0, 1, 1, 0, 1, 1], dtype=np.uint8)
    num, y, t = groupref.group_scan(sba, st, None, valid=valid, heads=heads)
    assert list(zip(num.tolist(), y.tolist(), t.tolist())) == [(1, 2, 2), (2, 2, 2), (4, 2, 2), (5, 2, 2), (6, 1, 1)]
    hist, total = groupref.group_scan(sba, st, None, valid=valid, heads=heads, max_counts_bin=1)
    assert hist.tolist() == [0, 3] and total == 5
    num, y, t = groupref.group_scan(sba, st, 2, valid=valid, is_sorted=False, yield_first_n=1)
    assert num.tolist() == [1, 2, 4, 5, 6] and set(t.tolist()) == {1}
    num, _, _ = groupref.group_scan(sba, st, 2, valid=np.zeros(8, dtype=bool))
    assert len(num) == 0
