"""The two-genome join on the device: gk_join through Kmers.count_in / compare / absent_from /
present_in and _native.Engine.join, on both paths (bytes, keys).

Every expectation comes from tests/joinref.py (numpy on the host sba: windows without '$', the
canonical form by a complement table spelt out there, np.unique and np.searchsorted on the rows in
byte order) and never from the code under test.  Every parametrised case first asserts on that
reference alone that it is not trivial -- shared, private-to-A and private-to-B k-mers wherever the
case intends them.  T mirrors the key path's tile (gkm_join_host.h: kTile merged elements per tile;
the mask kernel's tile of sorted positions has the same size).

One precondition has no case here: contexts on different devices need two GPUs.
"""

from functools import lru_cache

import numpy as np
import pytest

import joinref
from conftest import load_case, load_manifest, seq_list_of
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.sequence_collection import SequenceCollection

pytestmark = pytest.mark.gpu

T = 1024
CASES = {c["name"]: c for c in load_manifest()}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# genomes
# ---------------------------------------------------------------------------------------------
def rand_seq(seed, n, letters=b"ACGT") -> str:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


def mutate(seq: str, seed, every=37) -> str:
    """A substitution about every ``every`` bases (A->C->G->T->A)."""
    rng = np.random.default_rng(seed)
    s = bytearray(seq.encode())
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    for p in np.flatnonzero(rng.integers(0, every, len(s)) == 0).tolist():
        s[p] = nxt.get(s[p], 65)
    return s.decode()


def golden_seqs(name):
    case = CASES[name]
    return seq_list_of(case, load_case(name))


def one(seq):
    return [("c0", seq)]


def revcomp(s: str) -> str:
    return joinref.COMP[np.frombuffer(s.encode(), dtype=np.uint8)][::-1].tobytes().decode()


def is_acgt(seqs) -> bool:
    return all(set(s) <= set("ACGT") for _, s in seqs)


def keys_eligible(seqs_a, seqs_b, K, canonical=False, order="stable") -> bool:
    """The key path serves the pair: both ACGT-only, one length of at most 32 bases, a plain sort."""
    return is_acgt(seqs_a) and is_acgt(seqs_b) and K <= 32 and not canonical and order == "stable"


def sorted_kmers(seqs, K, canonical=False, order="stable"):
    sc = SequenceCollection(sequence_list=seqs, strands_to_load="forward")
    km = gk.Kmers(sc, min_kmer_len=K, max_kmer_len=K)
    km.sort(canonical=canonical, order=order)
    return km


def force(monkeypatch, path):
    if path == "auto":
        monkeypatch.delitem(_native.options, "GKM_JOIN_PATH", raising=False)
    else:
        monkeypatch.setitem(_native.options, "GKM_JOIN_PATH", path)


def check_join(km_a, km_b, ref, monkeypatch, paths):
    """count_in and compare on each path equal the reference; the result is aligned with
    get_unique_kmers."""
    for path in paths:
        force(monkeypatch, path)
        first, count = km_a.count_in(km_b)
        assert first.dtype == np.uint64 and count.dtype == np.uint32, path
        np.testing.assert_array_equal(count, ref["b_count"], err_msg=path)
        np.testing.assert_array_equal(first, ref["b_first"], err_msg=path)
        got = km_a.compare(km_b)
        assert {k: got[k] for k in joinref.STAT_NAMES} == ref["stats"], path
        assert {k: got[k] for k in ("jaccard", "containment")} == joinref.derived(ref["stats"]), path
    group_start, mult = km_a.get_unique_kmers()
    np.testing.assert_array_equal(mult, ref["a_count"])
    assert len(group_start) == len(ref["b_first"])


def run_pair(seqs_a, seqs_b, K, monkeypatch, canonical=False, order="stable", want=("shared", "only_a", "only_b")):
    """The whole check of one pair; ``want``: what the case intends to be non-empty."""
    ref = joinref.join(joinref.as_sba(seqs_a), joinref.as_sba(seqs_b), K, canonical)
    st = ref["stats"]
    have = {"shared": st["n_shared"], "only_a": st["n_distinct_a"] - st["n_shared"],
            "only_b": st["n_distinct_b"] - st["n_shared"]}
    for name in ("shared", "only_a", "only_b"):
        assert (have[name] > 0) == (name in want), (name, have)
    eligible = keys_eligible(seqs_a, seqs_b, K, canonical, order)
    km_a = sorted_kmers(seqs_a, K, canonical, order)
    km_b = km_a if seqs_b is seqs_a else sorted_kmers(seqs_b, K, canonical, order)
    check_join(km_a, km_b, ref, monkeypatch, ("auto", "bytes", "keys") if eligible else ("auto", "bytes"))
    if not eligible:
        force(monkeypatch, "keys")
        with pytest.raises(_native.GkError, match="GKM_JOIN_PATH=keys") as e:
            km_a.count_in(km_b)
        assert e.value.code == _native.GK_E_UNSUPPORTED
    force(monkeypatch, "auto")
    return ref, km_a, km_b


# ---------------------------------------------------------------------------------------------
# 1. small cases: the manifest's genomes against themselves and against each other
# ---------------------------------------------------------------------------------------------
SMALL = [
    ("seq2_min3_max3", "seq2_min3_max3", 3, ("shared",)),
    ("seq2_min3_max3", "seq2_min3_max3", 9, ("shared",)),
    ("seq2_min3_max3", "rand10k_k31", 4, ("shared", "only_b")),
    ("rand10k_k31", "seq2_min3_max3", 4, ("shared", "only_a")),
    ("rand10k_k31", "rand10k_k31", 31, ("shared",)),
    ("rand10k_k31", "c1_seed42_10kb_k5", 8, ("shared", "only_a", "only_b")),
    ("c1_seed42_10kb_k5", "rand10k_k31", 7, ("shared", "only_a", "only_b")),
    ("repeat_k31", "rand10k_k31", 6, ("shared", "only_a", "only_b")),
    ("repeat_k31", "repeat_k31", 31, ("shared",)),
    ("iupac_k31", "iupac_k31", 31, ("shared",)),
    ("iupac_k31", "rand10k_k31", 6, ("shared", "only_a", "only_b")),
    ("rand10k_k31", "iupac_k31", 6, ("shared", "only_a", "only_b")),
]


@pytest.mark.parametrize("name_a,name_b,K,want", SMALL, ids=[f"{a}-{b}-k{k}" for a, b, k, _ in SMALL])
def test_small_cases(name_a, name_b, K, want, monkeypatch):
    seqs_a = golden_seqs(name_a)
    seqs_b = seqs_a if name_b == name_a else golden_seqs(name_b)
    ref, km_a, km_b = run_pair(seqs_a, seqs_b, K, monkeypatch, want=want)
    if km_b is km_a:  # the identity: B's counts are A's own, B's insertion points A's group starts
        group_start, mult = km_a.get_unique_kmers()
        first, count = km_a.count_in(km_a)
        np.testing.assert_array_equal(count, mult)
        np.testing.assert_array_equal(first, group_start)
        st = km_a.compare(km_a)
        assert st["n_shared"] == st["n_distinct_a"] == st["n_distinct_b"] and st["jaccard"] == 1.0
        assert st["occ_a_shared"] == st["occ_b_shared"] == st["occ_min"] == len(km_a)


# ---------------------------------------------------------------------------------------------
# 2. tile-boundary sweep
# ---------------------------------------------------------------------------------------------
SWEEP = rand_seq(11, 3 * T + 15 + 70)  # about 3 T distinct 16-mers (plus a little: three full tiles of A alone)


@lru_cache(maxsize=None)
def sweep_kmers(j):
    return sorted_kmers(one(SWEEP[j:]), 16)


@pytest.mark.parametrize("swapped", [False, True], ids=["a-whole", "b-whole"])
@pytest.mark.parametrize("j", range(9))
def test_tile_boundary_sweep(j, swapped, monkeypatch):
    """B is A without its first j bases: all but j k-mers stay shared, and in the merged order every
    pair of equal keys after a missing one moves by one element, so over j = 0..8 the matches fall on
    both sides of every tile boundary.  With the roles swapped the missing k-mers are B's."""
    whole, cut = one(SWEEP), one(SWEEP[j:])
    a, b = (cut, whole) if swapped else (whole, cut)
    ref = joinref.join(joinref.as_sba(a), joinref.as_sba(b), 16)
    st = ref["stats"]
    assert st["n_distinct_a" if not swapped else "n_distinct_b"] >= 3 * T
    assert st["n_shared"] == min(st["n_distinct_a"], st["n_distinct_b"]) > 0
    assert abs(st["n_distinct_a"] - st["n_distinct_b"]) == j
    assert (st["n_distinct_a"] + st["n_distinct_b"]) // T >= 5  # several tiles
    km_a, km_b = (sweep_kmers(j), sweep_kmers(0)) if swapped else (sweep_kmers(0), sweep_kmers(j))
    check_join(km_a, km_b, ref, monkeypatch, ("keys", "bytes", "auto"))


# ---------------------------------------------------------------------------------------------
# 3. skew
# ---------------------------------------------------------------------------------------------
BIG = rand_seq(21, 30000)
TINY = BIG[12000:12025] + "ACGTTGCATTGACCA"  # 40 bases: the first k-mers are BIG's, the last are not
AC_ONLY, GT_ONLY = rand_seq(22, 3000, b"AC"), rand_seq(23, 3000, b"GT")


@pytest.mark.parametrize("a,b,K,want", [
    (BIG, TINY, 12, ("shared", "only_a", "only_b")),
    (TINY, BIG, 12, ("shared", "only_a", "only_b")),
    (AC_ONLY, GT_ONLY, 12, ("only_a", "only_b")),
    (GT_ONLY, AC_ONLY, 12, ("only_a", "only_b")),
], ids=["30kb-40b", "40b-30kb", "ac-gt", "gt-ac"])
def test_skew(a, b, K, want, monkeypatch):
    """Whole tiles hold one side only and the diagonal search ends on its clamps; with disjoint
    alphabets all of one side precedes the other and nothing is shared."""
    assert len(TINY) == 40
    ref, _, _ = run_pair(one(a), one(b), K, monkeypatch, want=want)
    assert ref["stats"]["n_distinct_a"] + ref["stats"]["n_distinct_b"] > T
    if "shared" not in want:
        assert set(ref["b_first"].tolist()) == {0 if a is AC_ONLY else len(b) - K + 1}


# ---------------------------------------------------------------------------------------------
# 4. extreme keys
# ---------------------------------------------------------------------------------------------
def test_extreme_keys(monkeypatch):
    """K = 32: poly-A (key 0) and poly-T (key 2^64 - 1) are ordinary shared k-mers."""
    K = 32
    common = rand_seq(31, 900)
    a = "A" * 40 + "C" + rand_seq(32, 1500) + common + "G" + "T" * 45 + "C" + rand_seq(33, 700)
    b = rand_seq(34, 1200) + "G" + "T" * 36 + "C" + common + rand_seq(35, 800) + "C" + "A" * 50
    ref, km_a, km_b = run_pair(one(a), one(b), K, monkeypatch)
    kmers = ref["a_kmers"].tolist()
    assert kmers[0] == b"A" * K and kmers[-1] == b"T" * K
    assert ref["a_count"][0] == 9 and ref["b_count"][0] == 19 and ref["b_first"][0] == 0
    assert ref["a_count"][-1] == 14 and ref["b_count"][-1] == 5 and ref["b_first"][-1] == len(b) - K + 1 - 5
    keys = km_a.get_encoded_kmers()
    assert int(keys.min()) == 0 and int(keys.max()) == 2 ** 64 - 1


# ---------------------------------------------------------------------------------------------
# 5. heavy groups
# ---------------------------------------------------------------------------------------------
HEAVY_X = "GATTACAGATCC"
HEAVY_N = T + 100
HEAVY_REST = rand_seq(41, 2500)
# one 12-mer more than T times (a contig each, so no other k-mer is repeated with it), then a random contig
HEAVY = [(f"x{i}", HEAVY_X) for i in range(HEAVY_N)] + [("rest", HEAVY_REST)]
LIGHT_WITH = one(rand_seq(42, 1500) + HEAVY_X + HEAVY_REST[300:900] + rand_seq(43, 800))
LIGHT_WITHOUT = one(rand_seq(42, 1500) + HEAVY_REST[300:900] + rand_seq(43, 800))


@pytest.mark.parametrize("a,b", [(LIGHT_WITH, HEAVY), (HEAVY, LIGHT_WITH), (HEAVY, LIGHT_WITHOUT)],
                         ids=["once-in-a", "once-in-b", "absent-from-b"])
def test_heavy_groups(a, b, monkeypatch):
    K = len(HEAVY_X)
    ref, km_a, km_b = run_pair(a, b, K, monkeypatch)
    u = ref["a_kmers"].tolist().index(HEAVY_X.encode())
    if a is HEAVY:
        assert ref["a_count"][u] == HEAVY_N > T and ref["b_count"][u] == (1 if b is LIGHT_WITH else 0)
    else:
        assert ref["a_count"][u] == 1 and ref["b_count"][u] == HEAVY_N
    # the mask over a group larger than its tile: occurrences, not distinct k-mers
    absent = int(ref["a_count"][ref["b_count"] == 0].sum())
    present = int(ref["a_count"][ref["b_count"] > 0].sum())
    assert absent > 0 and present > 0 and absent + present == len(km_a)
    for path in ("bytes", "keys"):
        force(monkeypatch, path)
        assert km_a.get_kmer_count(K, kmer_filter_func=km_a.absent_from(km_b)) == absent
        assert km_a.get_kmer_count(K, kmer_filter_func=km_a.present_in(km_b)) == present
    # group by group: a mask that cut the heavy group at a tile boundary would change its size
    for name, flag in (("absent_from", ref["b_count"] == 0), ("present_in", ref["b_count"] > 0)):
        hist, total = km_a.get_kmer_group_counts(K, kmer_filter_func=getattr(km_a, name)(km_b),
                                                 max_counts_bin=HEAVY_N + 1)
        assert total == int(ref["a_count"][flag].sum())
        np.testing.assert_array_equal(hist, np.bincount(ref["a_count"][flag], minlength=HEAVY_N + 2))


# ---------------------------------------------------------------------------------------------
# 6. inputs only the byte path serves
# ---------------------------------------------------------------------------------------------
def with_n_runs(seq: str, seed) -> str:
    """N runs and IUPAC letters over an ACGT sequence."""
    rng = np.random.default_rng(seed)
    s = bytearray(seq.encode())
    for p in rng.integers(0, len(s) - 40, 6).tolist():
        s[p:p + 25] = b"N" * 25
    for p, ch in zip(rng.integers(0, len(s), 12).tolist(), b"RYKMSWBDHVRY"):
        s[p] = ch
    return s.decode()


BASE = rand_seq(51, 4000)
MIXED_A = with_n_runs(BASE, 52)
MIXED_B = with_n_runs(mutate(BASE, 53), 52)  # the same N runs and letters: shared k-mers with N and IUPAC in them
PAL21 = "ACGGTCATGA" + "W" + revcomp("ACGGTCATGA")
PAL31 = "ACGGTCATGATTGCA" + "S" + revcomp("ACGGTCATGATTGCA")

BYTES_ONLY = {
    "mixed-mixed-k15": (one(MIXED_A), one(MIXED_B), 15, False, "stable"),
    "acgt-mixed-k15": (one(BASE), one(MIXED_B), 15, False, "stable"),
    "mixed-acgt-k15": (one(MIXED_A), one(mutate(BASE, 53)), 15, False, "stable"),
    "k40": (one(BASE), one(mutate(BASE, 54, every=90)), 40, False, "stable"),
    "k63": (one(BASE), one(mutate(BASE, 55, every=150)), 63, False, "stable"),
    "canonical-k21": (one(BASE[:1500] + PAL21 + BASE[1500:]),
                      one(revcomp(mutate(BASE, 56, every=60))[:2000] + PAL21 + rand_seq(57, 500)), 21, True, "stable"),
    "canonical-k31": (one(BASE[:1500] + PAL31 + BASE[1500:]),
                      one(revcomp(mutate(BASE, 58, every=90))[:2000] + PAL31 + rand_seq(59, 500)), 31, True, "stable"),
    "canonical-acgt-k21": (one(BASE), one(revcomp(mutate(BASE, 61, every=60))), 21, True, "stable"),
}


@pytest.mark.parametrize("case", list(BYTES_ONLY))
def test_bytes_only_inputs(case, monkeypatch):
    seqs_a, seqs_b, K, canonical, order = BYTES_ONLY[case]
    assert not keys_eligible(seqs_a, seqs_b, K, canonical, order)
    ref, _, _ = run_pair(seqs_a, seqs_b, K, monkeypatch, canonical=canonical, order=order)
    kmers = ref["a_kmers"].tolist()
    shared = {k for k, c in zip(kmers, ref["b_count"].tolist()) if c}
    if case == "mixed-mixed-k15":
        assert any(b"N" in k for k in shared) and any(set(k) & set(b"RYKMSWBDHV") for k in shared)
    if canonical:
        if "acgt" not in case:
            pal = (PAL21 if K == 21 else PAL31).encode()
            assert revcomp(pal.decode()).encode() == pal and pal in shared
        # B is mostly the reverse strand of A: shared only because both sides are canonical
        forward = joinref.join(joinref.as_sba(seqs_a), joinref.as_sba(seqs_b), K)
        assert forward["stats"]["n_shared"] < ref["stats"]["n_shared"] // 4


def test_reference_tie_order(monkeypatch):
    """sort(order="reference") permutes equal k-mers inside their groups only: the keys stay in sorted
    order and the unique view is the same, so every path serves it and gives the stable sort's join."""
    a, b = one(rand_seq(62, 3000)), one(mutate(rand_seq(62, 3000), 63))
    ref = joinref.join(joinref.as_sba(a), joinref.as_sba(b), 6)
    assert ref["stats"]["n_shared"] > 0 and int(ref["a_count"].max()) > 1
    check_join(sorted_kmers(a, 6, order="reference"), sorted_kmers(b, 6, order="reference"), ref, monkeypatch,
               ("auto", "bytes", "keys"))


# ---------------------------------------------------------------------------------------------
# 7. the Python surface: filters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["acgt-k8", "mixed-mixed-k15", "canonical-k21"])
def test_filters_give_the_private_and_the_shared_set(case, monkeypatch):
    if case == "acgt-k8":
        seqs_a, seqs_b, K, canonical = golden_seqs("rand10k_k31"), golden_seqs("c1_seed42_10kb_k5"), 8, False
    else:
        seqs_a, seqs_b, K, canonical, _ = BYTES_ONLY[case]
    ref = joinref.join(joinref.as_sba(seqs_a), joinref.as_sba(seqs_b), K, canonical)
    absent, present = ref["b_count"] == 0, ref["b_count"] > 0
    assert absent.any() and present.any()
    km_a, km_b = sorted_kmers(seqs_a, K, canonical), sorted_kmers(seqs_b, K, canonical)
    for name, flag in (("absent_from", absent), ("present_in", present)):
        filt = getattr(km_a, name)(km_b)
        assert km_a.get_kmer_count(K, kmer_filter_func=filt) == int(ref["a_count"][flag].sum())
        hist, total = km_a.get_kmer_group_counts(K, kmer_filter_func=filt, max_counts_bin=50)
        assert total == int(ref["a_count"][flag].sum())
        np.testing.assert_array_equal(hist[:50], np.bincount(ref["a_count"][flag], minlength=51)[:50])
        rows = list(km_a.get_kmers(K, kmer_filter_func=filt, yield_first_n=1))
        assert [t for _, _, t in rows] == ref["a_count"][flag].tolist()
        if not canonical:  # (a canonical k-mer may be read from the other strand: its string differs)
            got = [km_a.get_kmer_str(num, K).encode() for num, _, _ in rows]
            assert got == ref["a_kmers"][flag].tolist()
    # the filter sees `other` as it is when it is used, and serves its own Kmers and length only
    filt = km_a.absent_from(km_b)
    with pytest.raises(ValueError, match="another Kmers object"):
        km_b.get_kmer_count(K, kmer_filter_func=filt)
    if not canonical:
        with pytest.raises(ValueError, match=rf"max_kmer_len \({K}\) only \(kmer_len = {K - 1}\)"):
            km_a.get_kmer_count(K - 1, kmer_filter_func=filt)
    with pytest.raises(TypeError, match="cannot be called as"):
        filt(km_a.seq_coll.forward_sba, "forward", 0)
    with pytest.raises(ValueError, match="array-level functions"):
        gk.get_kmer_group_size_hist(km_a.seq_coll.forward_sba, "forward", K, km_a.kmer_sba_start_indices,
                                    gk.get_compare_sba_kmers_func(K), filt)
    # the built-in filters still work afterwards (the mask buffer is theirs again)
    assert km_a.get_kmer_count(K) == len(km_a)


# ---------------------------------------------------------------------------------------------
# 8. state and errors, through the engine
# ---------------------------------------------------------------------------------------------
def engine_of(seq: str, enumerate_k=None, sort_k="same", canonical=False):
    sba = joinref.as_sba(seq)
    eng = _native.Engine()
    eng.set_sequence(sba, np.concatenate([[0], np.flatnonzero(sba == joinref.DOLLAR) + 1]).astype(np.uint32))
    if enumerate_k is not None:
        eng.enumerate(enumerate_k)
        if sort_k != "no":
            eng.sort(enumerate_k if sort_k == "same" else sort_k, canonical=canonical)
    return eng


def join_error(a, b, code, match, flags=0):
    rc = a.lib.gk_join(a.ctx, b.ctx if b is not None else None, flags, None)
    assert rc == code, (rc, a.lib.gk_last_error(a.ctx))
    msg = a.lib.gk_last_error(a.ctx).decode()
    import re
    assert re.search(match, msg), msg


def test_preconditions_and_their_messages():
    E = _native
    s1, s2 = rand_seq(71, 600), rand_seq(72, 500)
    good = engine_of(s1, 12)
    other = engine_of(s2, 12)
    assert good.join(other)["n_distinct_a"] == len(set(s1[i:i + 12] for i in range(len(s1) - 11)))
    lib = good.lib
    assert lib.gk_join(None, good.ctx, 0, None) == E.GK_E_ARG
    join_error(good, None, E.GK_E_ARG, "null context b")
    join_error(good, other, E.GK_E_ARG, r"unknown flag bits \(flags = 4\)", flags=4)
    join_error(good, engine_of(s2, 9), E.GK_E_ARG, r"sort lengths differ \(a: 12, b: 9\)")
    join_error(good, engine_of(s2, 12, canonical=True), E.GK_E_ARG, r"a: forward, b: canonical")
    join_error(engine_of(s2, 12, canonical=True), good, E.GK_E_ARG, r"a: canonical, b: forward")
    join_error(good, _native.Engine(), E.GK_E_STATE, "no sequence loaded in context b")
    join_error(_native.Engine(), good, E.GK_E_STATE, "no sequence loaded in context a")
    join_error(good, engine_of(s2), E.GK_E_STATE, "context b are not sorted")
    join_error(good, engine_of(s2, 12, sort_k="no"), E.GK_E_STATE, "context b are not sorted")
    join_error(engine_of(s2, 12, sort_k="no"), good, E.GK_E_STATE, "context a are not sorted")
    join_error(engine_of(s1, 5, sort_k=None), engine_of(s2, 5, sort_k=None), E.GK_E_UNSUPPORTED,
               r"max_kmer_len None \(sort length 0\)")
    join_error(good, engine_of(s2, 5, sort_k=12), E.GK_E_UNSUPPORTED,
               r"context b holds k-mers cut short.*min_kmer_len = 5, sort length = 12")
    join_error(engine_of(s2, 5, sort_k=12), good, E.GK_E_UNSUPPORTED, r"context a holds k-mers cut short")
    # a refused join leaves no result behind
    assert lib.gk_join_mask(good.ctx, E.JOIN_KEEP_ABSENT) == E.GK_E_STATE
    # the knob: any other value is refused
    _native.options["GKM_JOIN_PATH"] = "both"
    try:
        join_error(good, other, E.GK_E_ARG, "GKM_JOIN_PATH must be 'bytes' or 'keys'")
    finally:
        del _native.options["GKM_JOIN_PATH"]


def test_result_state():
    E = _native
    s1, s2 = rand_seq(73, 700), rand_seq(74, 650)
    a, b = engine_of(s1, 10), engine_of(s2, 10)
    lib = a.lib
    first = np.zeros(4096, dtype=np.uint64)
    count = np.zeros(4096, dtype=np.uint32)
    pf, pc = first.ctypes.data_as(E._U64P), count.ctypes.data_as(E._U32P)
    for call in (lambda: lib.gk_copy_join(a.ctx, pf, pc, 1), lambda: lib.gk_device_join(a.ctx, None, None, None),
                 lambda: lib.gk_join_mask(a.ctx, E.JOIN_KEEP_ABSENT)):
        assert call() == E.GK_E_STATE and b"gk_join first" in lib.gk_last_error(a.ctx)
    st = a.join(b)
    ref = joinref.join(s1, s2, 10)
    assert st == ref["stats"]
    na = st["n_distinct_a"]
    got_first, got_count = a.join_result()
    np.testing.assert_array_equal(got_first, ref["b_first"])
    np.testing.assert_array_equal(got_count, ref["b_count"])
    # a wrong n; either array may be left out
    assert lib.gk_copy_join(a.ctx, pf, pc, na + 1) == E.GK_E_ARG
    assert f"n ({na + 1}) differs from the distinct k-mer count ({na})".encode() in lib.gk_last_error(a.ctx)
    assert lib.gk_copy_join(a.ctx, pf, pc, na - 1) == E.GK_E_ARG
    assert lib.gk_copy_join(a.ctx, None, pc, na) == E.GK_OK
    np.testing.assert_array_equal(count[:na], ref["b_count"])
    # the device view
    import ctypes
    df, dc, dn = E._P(), E._P(), ctypes.c_uint64()
    assert lib.gk_device_join(a.ctx, ctypes.byref(df), ctypes.byref(dc), ctypes.byref(dn)) == E.GK_OK
    assert dn.value == na and df.value and dc.value and df.value != dc.value
    # the mask's keep values
    for keep in (0, 3, -1):
        assert lib.gk_join_mask(a.ctx, keep) == E.GK_E_ARG
        assert f"keep ({keep})".encode() in lib.gk_last_error(a.ctx)
    assert lib.gk_join_mask(a.ctx, E.JOIN_KEEP_PRESENT) == E.GK_OK
    # the result is B's snapshot: B may go away or change
    b.sort(10)
    np.testing.assert_array_equal(a.join_result()[1], ref["b_count"])
    # ... but it goes with A's unique view: a re-sort, new start indices
    a.sort(10)
    assert lib.gk_copy_join(a.ctx, pf, pc, na) == E.GK_E_STATE
    assert lib.gk_join_mask(a.ctx, E.JOIN_KEEP_ABSENT) == E.GK_E_STATE
    assert a.unique_count_only() == na  # the view alone does not bring the join back
    assert lib.gk_copy_join(a.ctx, pf, pc, na) == E.GK_E_STATE
    assert a.join(b) == ref["stats"]
    a.set_start_indices(np.arange(len(s1) - 9, dtype=np.uint32), 10)
    assert lib.gk_copy_join(a.ctx, pf, pc, na) == E.GK_E_STATE
    assert lib.gk_join_mask(a.ctx, E.JOIN_KEEP_ABSENT) == E.GK_E_STATE
    a.sort(10)
    assert a.join(b) == ref["stats"]
    # a group pass rewrites the view's buffers: the join goes too
    a.group_hist(True, 10, E.GkFilter(E.FILTER_KEEP_ALL, 0, 0, 0, 0), 1, None, 10)
    assert lib.gk_copy_join(a.ctx, pf, pc, na) == E.GK_E_STATE


def test_empty_and_single_kmer_sides():
    s = rand_seq(75, 400)
    full = engine_of(s, 10)
    ref = joinref.join(s, s, 10)
    empty = engine_of(s)
    empty.set_start_indices(np.empty(0, dtype=np.uint32), 10)
    empty.sort(10)
    zeros = dict.fromkeys(joinref.STAT_NAMES, 0)
    assert empty.join(full) == zeros | {"n_distinct_b": ref["stats"]["n_distinct_a"]}
    first, count = empty.join_result()
    assert len(first) == 0 and len(count) == 0
    assert empty.join(empty) == zeros
    assert full.join(empty) == zeros | {"n_distinct_a": ref["stats"]["n_distinct_a"]}
    first, count = full.join_result()
    assert not first.any() and not count.any() and len(first) == ref["stats"]["n_distinct_a"]
    # one k-mer: the sort leaves it without keys
    single = engine_of(s)
    single.set_start_indices(np.array([37], dtype=np.uint32), 10)
    single.sort(10)
    want = joinref.join(s[37:47], s, 10)
    assert want["stats"]["n_shared"] == 1
    assert single.join(full) == want["stats"]
    first, count = single.join_result()
    np.testing.assert_array_equal(first, want["b_first"])
    np.testing.assert_array_equal(count, want["b_count"])
    back = joinref.join(s, s[37:47], 10)
    assert full.join(single) == back["stats"]
    np.testing.assert_array_equal(full.join_result()[0], back["b_first"])
    np.testing.assert_array_equal(full.join_result()[1], back["b_count"])
