"""gk_sort's variable-length and suffix-order paths (min_kmer_len < max_kmer_len: bounded keys;
max_kmer_len None: prefix doubling; bounds beyond 256-bit keys: capped doubling; user-given starts) at
tile, word and round edges: the inputs of tests/edgegen.py through both routes of the key sorts, against
the CPU oracle alone.

Tiles: 4,096 positions in the position encoders (gkm_encode.hip kEncodeTile), in the LSD onesweep of
keys of two or more words and in the flag scans (kScanTile); 12,288 keys in the onesweep of one-word
keys; n1 = 8,191 / 8,192 / 8,193 positions is where the doubling's rank width changes.  Bounds: every
max at which the key takes another word (ACGT: 2 max + bit_width(max) bits; IUPAC: 4 max) and the
first bound past 256 bits.  Each test is one (route, alphabet, bounds, builder, builder's k, T) and
loops over the builder's arrays, a fresh engine per array; the array's label is in every assertion
message, and the route is asserted for every array from its own timers.  The oracle's answers are
cached per (alphabet, bounds, builder, k, T): the routes share them.

Routes: "lsd" pins the LSD passes (GKM_SORT_KEYS_LSD=1, the default at these sizes); "msd" lowers
the size from which the large-array routes run to 2 (GKM_MSD_KEYS_MIN): MSD levels over one-word keys,
doubling rounds over the tied groups only, bounded ACGT keys of two or more words through capped
doubling with the keys re-derived.  IUPAC keys of two or more words have no MSD levels (sort_keys_msd
takes one-word keys only): their "msd" tests assert that the LSD passes ran.

Checked per array: the enumerated starts, the sorted starts, the key layout, the keys -- encoded keys
against oracle.encode_keys; ranks (layout bits 0) non-decreasing and equal between neighbours exactly
where oracle.compare says the k-mers are equal, which every finish of the doubling promises (in
place and keep_long_enough carry the last round's keys, equal iff the symbols compared are; the sort
of user-given starts reads dense group ranks; the rounds over tied groups number the groups) -- the
group histogram at max (min under None) and the unique counts.
"""

import collections
import ctypes
import functools

import numpy as np
import pytest

import edgegen
from genome_kmers import _native
from genome_kmers import kmers as gk
from oracle import oracle

pytestmark = pytest.mark.gpu

T_ENC, T_RANK, T_ONE = 4096, 8192, 12288
BIN = 64  # last bin of the group histograms
ROUTES = {"lsd": {"GKM_SORT_KEYS_LSD": "1"}, "msd": {"GKM_MSD_KEYS_MIN": "2"}}

# (min, max): ACGT keys hold 2 max + bit_width(max) bits -- 29 | 30, 61 | 62, 92 | 93 are the last bound
# of a word and the first of the next, 124 the last direct key, 125 the first capped doubling; IUPAC keys
# 4 max bits -- 16 | 17, 32 | 33, 48 | 49, and 64 | 65 for the doubling with the 16-symbol seed
BOUNDS = {
    "acgt": [(1, 29), (5, 29), (5, 30), (5, 61), (5, 62), (5, 92), (5, 93), (5, 124), (5, 125), (1, None), (5, None),
             (40, None)],
    "iupac": [(3, 16), (3, 17), (3, 32), (3, 33), (3, 48), (3, 49), (3, 64), (3, 65), (1, None), (3, None)],
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


def key_words(acgt, lo, hi):
    return None if hi is None else oracle.key_spec(acgt, lo, hi)[3]


def is_doubling(acgt, lo, hi):
    """the keys are ranks: no bound, or a bound beyond four key words"""
    return hi is None or key_words(acgt, lo, hi) > 4


# ---------------------------------------------------------------------------------------------
# inputs and their oracle answers
# ---------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "label sba seg unsorted want spec keys ties hist total uhist")


def inputs(builder, kb, T, acgt):
    kw = {}
    if builder == "shared_tails":
        kw["tails"] = edgegen.TAILS_ACGT if acgt else edgegen.TAILS_IUPAC
    if builder == "separators3":
        # the arrays for the user-given starts: the '$' around 3 T, so that more than 12,288 starts exist
        builder, kw = "separators", {"tiles": (3,)}
        arrays = [a for a in edgegen.separators(kb, T, **kw) if a[0].startswith("sep-")]
    else:
        args = (kb,) if T is None else (kb, T)
        arrays = getattr(edgegen, builder)(*args, **kw)
    return arrays if acgt else edgegen.iupac(arrays, edgegen.planted(builder, kb, T, **kw))


def oracle_ties(label, sba, order, hi):
    """ties[i]: oracle.compare(sba, order[i - 1], order[i], hi)[0] == 0 (ties[0] False) -- gko_compare
    called with the arguments oracle.compare passes, the pointers made once"""
    lib = oracle.lib()
    sba = np.ascontiguousarray(sba, dtype=np.uint8)
    ptr, n, m, last = sba.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), sba.size, -1 if hi is None else hi, ctypes.c_int64(0)
    ref = ctypes.byref(last)
    o = order.tolist()
    ties = np.zeros(len(o), dtype=bool)
    for i in range(1, len(o)):
        r = lib.gko_compare(ptr, n, o[i - 1], o[i], m, ref)
        assert r in (-1, 0), (label, i, r)  # the oracle's own order
        ties[i] = r == 0
    return ties


def answers(label, sba, seg, unsorted, start_set, lo, hi, acgt):
    """the oracle's answers for the sort of start_set (ascending) under (lo, hi)"""
    want = oracle.quicksort(sba, start_set, lo, hi, break_ties=True)
    if is_doubling(acgt, lo, hi):
        spec, keys, ties = None, None, oracle_ties(label, sba, want, hi)
    else:
        spec = oracle.key_spec(acgt, lo, hi)
        keys, ties = oracle.encode_keys(sba, want, *spec), None
    hist, total = oracle.group_scan(sba, want, lo if hi is None else hi, max_counts_bin=BIN)
    uhist, _ = oracle.group_scan(sba, want, hi, max_counts_bin=BIN)
    for a in (sba, seg, unsorted, want, keys, ties):
        if a is not None:
            a.setflags(write=False)
    return Ref(label, sba, seg, unsorted, want, spec, keys, ties, hist, total, uhist)


@functools.lru_cache(maxsize=2)
def reference(acgt, lo, hi, builder, kb, T):
    """Consecutive tests share the arguments: the parameter lists below are ordered for that."""
    out = []
    for label, sba, seg in inputs(builder, kb, T, acgt):
        unsorted = oracle.enumerate_starts(sba, seg, lo)
        out.append(answers(label, sba, seg, unsorted, unsorted, lo, hi, acgt))
    return out


# ---------------------------------------------------------------------------------------------
# one sort, checked
# ---------------------------------------------------------------------------------------------
def sort_and_check(r, lo, hi, acgt, tag, route, tied=False, user=None):
    """r: the answers for the enumeration, or -- user: the starts as given -- for that set; route,
    tied: what assert_route checks from this sort's timers"""
    tag = f"{tag} {r.label}"
    eng = _native.Engine()
    eng.set_sequence(r.sba, r.seg)
    assert eng.is_acgt() == acgt, tag
    if user is None:
        n = eng.enumerate(lo)
        assert n == len(r.unsorted), tag
        np.testing.assert_array_equal(eng.copy_starts(), r.unsorted, err_msg=tag + ": enumerated starts")
    else:
        eng.set_start_indices(user, lo)
        n = len(user)
    eng.profile_enable(True)
    eng.sort(hi)
    timers = set(eng.profile_report().keys())
    eng.profile_enable(False)
    # first the width the sort ran at (the layout exists once a sort has finished), then its route
    words, bits, symbols = eng.key_layout()
    if r.spec is not None:
        assert (words, bits, symbols) == (r.spec[3], r.spec[0], r.spec[1]), tag
    else:
        assert (words, bits, symbols) == (1, 0, 0), tag
    assert_route(route, acgt, lo, hi, timers, tag, tied=tied,
                 user=None if user is None else 2 * len(user) >= len(r.sba))
    got = eng.copy_starts()
    np.testing.assert_array_equal(got, r.want, err_msg=tag + ": sorted starts")
    if r.spec is not None:
        keys = eng.copy_keys()
        np.testing.assert_array_equal(keys, r.keys.reshape(keys.shape), err_msg=tag + ": keys")
    else:
        ranks = eng.copy_keys().ravel()
        assert (ranks[1:] >= ranks[:-1]).all(), tag + ": ranks decrease along the sorted order"
        np.testing.assert_array_equal(ranks[1:] == ranks[:-1], r.ties[1:], err_msg=tag + ": equal ranks vs equal k-mers")
    hist, total = eng.group_hist(True, lo if hi is None else hi, gk.kmer_filter_keep_all.gk_filter(), 1, None, BIN)
    np.testing.assert_array_equal(hist, r.hist, err_msg=tag + ": group histogram")
    assert total == r.total == n, tag
    first, counts = eng.unique_counts()
    assert int(counts.sum()) == n, tag
    np.testing.assert_array_equal(first, np.cumsum(counts, dtype=np.uint64) - counts, err_msg=tag + ": unique firsts")
    np.testing.assert_array_equal(np.bincount(np.minimum(counts, BIN), minlength=BIN + 1), r.uhist,
                                  err_msg=tag + ": unique counts")
    return got


def assert_route(route, acgt, lo, hi, timers, tag, tied=False, user=None):
    """The route named ran, from one sort's timers: radix_pass is radix_sort's passes, msd_total the
    MSD levels over keys (msd_sort_keys), msd_groups a doubling round over the tied groups
    (msd_sort_groups).  tied: the array keeps groups tied behind the seed key.  user: None for the
    enumeration, else whether the given starts cover half the positions -- only then does gk_sort
    reroute bounded keys of two or more words through the capped doubling; a smaller set keeps the
    direct keys, which have no MSD levels."""
    seen = (tag, sorted(timers))
    words = key_words(acgt, lo, hi)
    multiword_direct = words is not None and 2 <= words <= 4 and (not acgt or user is False)
    if route == "lsd" or multiword_direct:
        assert "radix_pass" in timers and not {"msd_total", "msd_groups"} & timers, seen
        return
    assert "msd_total" in timers, seen
    if user is None:  # (user-given starts are ordered by position first: LSD passes on any route)
        assert "radix_pass" not in timers, seen
    if tied and (is_doubling(acgt, lo, hi) or words >= 2):
        assert "msd_groups" in timers, seen


# ---------------------------------------------------------------------------------------------
# the whole enumeration
# ---------------------------------------------------------------------------------------------
def enumeration_params():
    rows = []
    for a, alpha in enumerate(BOUNDS):
        acgt = alpha == "acgt"
        for lo, hi in BOUNDS[alpha]:
            words = key_words(acgt, lo, hi)
            tiles = [T_ENC] + ([T_RANK] if hi is None else []) + ([T_ONE] if hi is None or words == 1 else [])
            # k = min: every contig must hold min bases; k = max: the '$' offsets and the contig of
            # exactly k bases against the full window
            for kb in [lo] + ([hi] if hi is not None else []):
                rows += [(a, lo, hi, builder, kb, T) for builder in ("ends", "separators") for T in tiles]
                if kb <= edgegen.COMB_LEN:
                    rows.append((a, lo, hi, "comb", kb, None))
            rows += [(a, lo, hi, builder, lo, None) for builder in ("long_ties", "shared_tails")]
    out = []
    for a, lo, hi, builder, kb, T in rows:
        alpha = list(BOUNDS)[a]
        for route in ROUTES:
            name = f"{route}-{alpha}-{lo}_{hi}-{builder}" + ("" if kb == lo else "-kmax") + (f"-T{T}" if T else "")
            out.append(pytest.param(route, alpha, lo, hi, builder, kb, T, id=name))
    return out


@pytest.mark.parametrize("route,alpha,lo,hi,builder,kb,T", enumeration_params())
def test_varlen_edges(route, alpha, lo, hi, builder, kb, T, monkeypatch):
    acgt = alpha == "acgt"
    for name, value in ROUTES[route].items():
        monkeypatch.setitem(_native.options, name, value)
    tag = f"{route} {alpha} ({lo}, {hi}) {builder} k={kb} T={T}"
    for r in reference(acgt, lo, hi, builder, kb, T):
        sort_and_check(r, lo, hi, acgt, tag, route, tied=builder == "long_ties")


# ---------------------------------------------------------------------------------------------
# user-given starts
# ---------------------------------------------------------------------------------------------
# subsets around the 12,288-key tile of presort_by_start's one-word passes, and a small one
USER_SIZES = (12287, 12288, 12289, 700)
USER_BOUNDS = {"one-word": (5, 29), "multi-word": (5, 62), "none": (3, None)}


@functools.lru_cache(maxsize=1)
def user_reference(lo, hi):
    """[(answers, starts as given)]: per array one of the tile sizes and the small one; shared by the
    routes (the parameters below run a kind's routes back to back)"""
    out = []
    for i, r in enumerate(reference(True, lo, hi, "separators3", lo, T_ENC)):
        assert len(r.unsorted) >= max(USER_SIZES), r.label
        perm = np.random.default_rng([11, i]).permutation(r.unsorted)
        for size in USER_SIZES[i % 3:i % 3 + 1] + USER_SIZES[3:]:
            user = perm[:size].astype(np.uint32)
            user.setflags(write=False)
            out.append((answers(f"{r.label} {size} starts", r.sba, r.seg, r.unsorted, np.sort(user), lo, hi, True), user))
    return out


@pytest.mark.parametrize("kind", list(USER_BOUNDS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_user_starts_edges(route, kind, monkeypatch):
    """A seeded permutation of a subset of the enumeration, as the starts; expected
    oracle.quicksort(sba, np.sort(user), min, max, break_ties=True).  Subsets of 12,287 and more cover
    most positions: the "msd" route takes multi-word bounded keys through the capped doubling and
    sorts the starts by their final ranks (sort_user_starts), as under None; the small subset keeps
    the direct keys."""
    lo, hi = USER_BOUNDS[kind]
    for name, value in ROUTES[route].items():
        monkeypatch.setitem(_native.options, name, value)
    tag = f"user starts {route} ({lo}, {hi})"
    for ru, user in user_reference(lo, hi):
        sort_and_check(ru, lo, hi, True, tag, route, user=user)
