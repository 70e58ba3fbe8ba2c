"""gk_sort's position kernels at tile, word and k edges: the inputs of tests/edgegen.py (a '$', a
run of one non-ACGT letter, a single IUPAC letter or the end of the array placed around a tile edge
on purpose; tests/test_edgegen.py pins where) through every L0 path, bit-exact against the CPU oracle.

Tiles: 24,576 positions in the L0 count and partition kernels (gkm_msd_l0.h kP0Tile), 18,432 in the
wide L0, 8,192 in the split sort's class-B flag pass (gkm_split.hip kFlagTile), 4,096 in the
key-range select; every builder is called with the tile of the kernel under test.  Each test is one
(path, k, builder) and loops over the builder's arrays, a fresh engine per array; the array's label
is in every assertion message.

Checked per array -- forward: the enumerated starts (oracle.enumerate_starts), the sorted starts
(oracle.quicksort, break_ties=True), the keys (oracle.encode_keys), the group histogram
(oracle.group_scan) and the unique counts against that histogram; canonical: oracle.canonical_sort,
canonical_keys, canonical_windows (strands) and canonical_group_hist.
"""

import collections
import functools

import numpy as np
import pytest

import edgegen
from genome_kmers import _native
from genome_kmers import distributed as D
from genome_kmers import kmers as gk
from oracle import oracle

pytestmark = pytest.mark.gpu

T_L0, T_WIDE, T_FLAG, T_SELECT, T_XFER = 24576, 18432, 8192, 4096, 65536
BIN = 64  # last bin of the group histograms


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _native.device_count() > 0, "gpu tests need a visible MI355X"


# ---------------------------------------------------------------------------------------------
# inputs and their oracle answers, computed once per (builder, k, T) and shared by the paths
# ---------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "label sba seg unsorted want keys strands hist total")


def inputs(builder, k, T):
    if builder == "comb":
        return edgegen.comb(k)
    if builder == "runs-l0":
        # the class-A L0 of the split sort (24,576), where every non-ACGT byte is a stop: the shortest,
        # a middle and the longest run at every fixed placement, three of the straddling splits, the
        # single letters and the other extras (the flag pass's own tile has the full set, at 8,192)
        return edgegen.runs(k, T, lengths=(k - 1, k + 1, 64 + k), splits=(1, 17, 33))
    return getattr(edgegen, builder)(k, T)


@functools.lru_cache(maxsize=3)
def reference(builder, k, T, canonical, acgt):
    """Consecutive tests share (builder, k, T): the parameter lists below are ordered for that."""
    out = []
    bits = 2 if acgt else 4
    for label, sba, seg in inputs(builder, k, T):
        unsorted = oracle.enumerate_starts(sba, seg, k)
        if canonical:
            want = oracle.canonical_sort(sba, unsorted, k)
            keys = oracle.canonical_keys(sba, want, k, bits)
            strands = oracle.canonical_windows(sba, want, k)[1].astype(np.uint8)
            hist, total = oracle.canonical_group_hist(sba, want, k, BIN)
        else:
            want = oracle.quicksort(sba, unsorted, k, k, break_ties=True)
            keys = oracle.encode_keys(sba, want, *oracle.key_spec(acgt, k, k))
            strands = None
            hist, total = oracle.group_scan(sba, want, k, max_counts_bin=BIN)
        for a in (sba, seg, unsorted, want, keys):
            a.setflags(write=False)
        out.append(Ref(label, sba, seg, unsorted, want, keys, strands, hist, total))
    return out


def load(r, monkeypatch, packed=False):
    """A fresh engine holding r's sequence; packed: through the packed transfer, one 64 KiB block per
    chunk (as tests/test_gpu_xfer.py sets it), which leaves the resident 2-bit copy."""
    if packed:
        monkeypatch.setenv("GKM_PACK_MIN", "0")
        monkeypatch.setenv("GKM_PACK_BLOCKS", "1")
        monkeypatch.setenv("GKM_XFER_THREADS", "2")
    eng = _native.Engine()
    eng.set_sequence(r.sba, r.seg)
    for v in ("GKM_PACK_MIN", "GKM_PACK_BLOCKS", "GKM_XFER_THREADS"):
        monkeypatch.delenv(v, raising=False)
    return eng


def sort_and_check(eng, r, k, canonical, acgt, tag, timers=None):
    tag = f"{tag} {r.label}"
    n = eng.enumerate(k)
    assert n == len(r.unsorted), tag
    np.testing.assert_array_equal(eng.copy_starts(), r.unsorted, err_msg=tag + ": enumerated starts")
    assert eng.is_acgt() == acgt, tag
    if timers is not None:
        eng.profile_enable(True)
    eng.sort(k, canonical=canonical)
    if timers is not None:
        timers.update(eng.profile_report().keys())
        eng.profile_enable(False)
    np.testing.assert_array_equal(eng.copy_starts(), r.want, err_msg=tag + ": sorted starts")
    spec = oracle.key_spec(acgt, k, k)
    assert eng.key_layout() == (spec[3], spec[0], spec[1]), tag
    got = eng.copy_keys()
    np.testing.assert_array_equal(got, r.keys.reshape(got.shape), err_msg=tag + ": keys")
    if canonical:
        np.testing.assert_array_equal(eng.copy_strands(), r.strands, err_msg=tag + ": strands")
    hist, total = eng.group_hist(True, k, gk.kmer_filter_keep_all.gk_filter(), 1, None, BIN)
    np.testing.assert_array_equal(hist, r.hist, err_msg=tag + ": group histogram")
    assert total == r.total == n, tag
    first, counts = eng.unique_counts()
    np.testing.assert_array_equal(np.bincount(np.minimum(counts, BIN), minlength=BIN + 1), r.hist,
                                  err_msg=tag + ": unique counts")
    np.testing.assert_array_equal(first, np.cumsum(counts, dtype=np.uint64) - counts, err_msg=tag + ": unique firsts")
    assert int(counts.sum()) == n, tag
    return eng.copy_starts()


# ---------------------------------------------------------------------------------------------
# ACGT sba: the 2-bit L0 paths
# ---------------------------------------------------------------------------------------------
# path -> (tile, k's, library options, packed transfer)
FORWARD_PATHS = {
    # k = 3, 4: keys narrower than the 7-bit L0 digit; 55, 56 | 57: win8_keep's stop-window switch
    # (gkm_msd_l0.h, a.symbols <= 56); 32 | 33 and 63, 64: the ends of the first and second key word
    "default": (T_L0, [3, 4, 8, 31, 32, 33, 55, 56, 57, 63, 64], {}, False),
    # the 11-byte packed L0 output, read back by a pair level (l1_pairs) or expanded (l1_plain)
    "p88-l1_pairs": (T_L0, [24, 31, 32], {"GKM_TEST_P88": "1", "GKM_TEST_PAIRS": "1"}, False),
    "p88-l1_plain": (T_L0, [24, 31, 32], {"GKM_TEST_P88": "1"}, False),
    "wide": (T_WIDE, [10, 31, 32], {"GKM_WIDE_L0": "1"}, False),
    "resident": (T_L0, [31, 32, 57], {}, True),
}
CANONICAL_PATHS = {
    # k = 3 | 4: the canonical count kernel's fast path needs symbols >= 4
    "default": (T_L0, [3, 4, 31, 32, 33, 56, 57, 63, 64], {}, False),
    "resident": (T_L0, [32], {}, True),
}


def path_params(paths):
    """(path, k, builder, T), ordered so that the tests sharing an oracle answer run back to back"""
    rows = []
    for path, (T, ks, _, packed) in paths.items():
        for k in ks:
            for builder in ("ends", "separators", "comb"):
                rows.append((T, k, builder, path))
            if packed:  # the end of the array against the packed words, the '$' on the ends of a transfer block
                rows.append((T_XFER, k, "tails", path))
    rows.sort(key=lambda r: (r[0], r[1], r[2], list(paths).index(r[3])))
    return [pytest.param(path, k, builder, T, id=f"{path}-k{k}-{builder}") for T, k, builder, path in rows]


def run_acgt_path(paths, path, k, builder, T, canonical, monkeypatch):
    _, _, options, packed = paths[path]
    for name, value in options.items():
        monkeypatch.setitem(_native.options, name, value)
    if "GKM_TEST_P88" in options and k == 32:
        # 64 - 7 - 8 = 49 bits do not fit the packed pair; with an 8-bit L0 48 do (as test_packed_l0_vs_oracle)
        monkeypatch.setitem(_native.options, "GKM_LEVEL_BITS", "8,8,8")
    tag = f"{'canonical' if canonical else 'forward'} {path} k={k}"
    timers = set()
    for r in reference(builder, k, T, canonical, True):
        eng = load(r, monkeypatch, packed)
        if packed:
            assert eng.resident_packed(), tag
        got = sort_and_check(eng, r, k, canonical, True, tag, timers)
        if packed:  # the same sort with the L0 packing the bytes per tile
            monkeypatch.setenv("GKM_NO_RESIDENT_PACK", "1")
            plain = load(r, monkeypatch, True)
            monkeypatch.delenv("GKM_NO_RESIDENT_PACK")
            assert not plain.resident_packed(), tag
            plain.enumerate(k)
            plain.sort(k, canonical=canonical)
            np.testing.assert_array_equal(plain.copy_starts(), got, err_msg=f"{tag} {r.label}: without the resident copy")
    if "GKM_TEST_P88" in options:
        assert "msd_pass_l0k" in timers, (tag, sorted(timers))  # the L0 wrote the packed output
    else:
        assert "msd_pass_l0" in timers, (tag, sorted(timers))


@pytest.mark.parametrize("path,k,builder,T", path_params(FORWARD_PATHS))
def test_forward_acgt_edges(path, k, builder, T, monkeypatch):
    run_acgt_path(FORWARD_PATHS, path, k, builder, T, False, monkeypatch)


@pytest.mark.parametrize("path,k,builder,T", path_params(CANONICAL_PATHS))
def test_canonical_acgt_edges(path, k, builder, T, monkeypatch):
    run_acgt_path(CANONICAL_PATHS, path, k, builder, T, True, monkeypatch)


# ---------------------------------------------------------------------------------------------
# mixed sba: the split sort (class-B flag pass, class-A L0 with non-ACGT stops)
# ---------------------------------------------------------------------------------------------
MIXED_KS = [4, 16, 17, 31, 32, 33, 56, 57, 63]


@pytest.mark.parametrize("canonical", [False, True], ids=["fwd", "canon"])
@pytest.mark.parametrize("builder,T", [("runs", T_FLAG), ("runs-l0", T_L0)], ids=["flag8192", "l0_24576"])
@pytest.mark.parametrize("k", MIXED_KS)
def test_mixed_runs_edges(k, builder, T, canonical, monkeypatch):
    tag = f"mixed {'canonical' if canonical else 'forward'} T={T} k={k}"
    timers = set()
    for r in reference(builder, k, T, canonical, False):
        sort_and_check(load(r, monkeypatch), r, k, canonical, False, tag, timers)
    # the split sort ran (few class-B k-mers), with homopolymer groups from the planted runs of >= k letters
    assert {"split_b_select", "split_merge", "split_b_homo"} <= timers, (tag, sorted(timers))


@pytest.mark.parametrize("canonical", [False, True], ids=["fwd", "canon"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_mixed_runs_k3(k, canonical, monkeypatch):
    """k <= 3: 4-bit keys of at most 12 bits, the class-A keys narrower than the 7-bit L0 digit; the
    key-range shards take no split below k = 4 (gkm_shard.hip range_split), gk_sort decides by the
    class-B share.  k = 1: every class-B k-mer is a homopolymer, so the split sort has no B starts to
    sort and goes from the select to the homopolymer splice; k = 2, 3: the select kernel's short-k
    branches"""
    tag = f"mixed {'canonical' if canonical else 'forward'} k={k}"
    timers = set()
    for r in reference("runs", k, T_FLAG, canonical, False):
        sort_and_check(load(r, monkeypatch), r, k, canonical, False, tag, timers)
    assert {"split_b_select", "split_merge", "split_b_homo"} <= timers, (tag, sorted(timers))  # the split sort ran


# ---------------------------------------------------------------------------------------------
# key-range shards: histogram and select over 4,096-position tiles
# ---------------------------------------------------------------------------------------------
CODE = np.full(256, 255, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i


def digit_histogram(sba, k, lo, hi, bits):
    """numpy: the top `bits` bits of the 2-bit keys of the ACGT-only k-mers starting in [lo, hi)"""
    c = CODE[sba]
    p = np.arange(lo, max(lo, min(hi, len(sba) - k + 1)))
    ok = np.ones(len(p), dtype=bool)
    dig = np.zeros(len(p), dtype=np.int64)
    for j in range(k):
        cj = c[p + j]
        ok &= cj != 255
        if 2 * j < bits:
            dig = (dig << 2) | np.where(cj == 255, 0, cj)
    return np.bincount(dig[ok], minlength=1 << bits)


def shares(L, T):
    """[lo, hi) with lo a multiple of 32 (gk_shard_histogram's contract) and hi on T - 1, T, T + 1 and
    on a multiple of 32 - 1, + 1"""
    his = [T - 1, T, T + 1, T + 32 * 5 - 1, T + 32 * 5 + 1, L]
    los = [0, 32, 0, T - 64, 64, T]
    return [(lo, hi) for lo, hi in zip(los, his) if lo < hi <= L]


def class_b_starts(sba, seg, k, lo, hi):
    """(non-homopolymer, homopolymer) class-B starts in [lo, hi), ascending"""
    from numpy.lib.stride_tricks import sliding_window_view
    starts = oracle.enumerate_starts(sba, seg, k).astype(np.int64)
    starts = starts[(starts >= lo) & (starts < hi)]
    win = sliding_window_view(sba, k)[starts]
    class_b = (CODE[win] == 255).any(axis=1)
    homo = (win == win[:, :1]).all(axis=1) & class_b
    return starts[class_b & ~homo], starts[homo]


@pytest.mark.parametrize("builder", ["separators", "comb", "runs"])
@pytest.mark.parametrize("k", [31, 57])
def test_key_range_shards_edges(k, builder, monkeypatch):
    world = 3
    mixed = builder == "runs"
    tag = f"shards k={k} {builder}"
    for r in reference(builder, k, T_SELECT, False, not mixed):
        L = len(r.sba)
        eng = load(r, monkeypatch)
        bits = min(12, 2 * k)
        for lo, hi in shares(L, T_SELECT):
            h, b = eng.shard_histogram(lo, hi, k)
            assert b == bits, (tag, r.label)
            want = digit_histogram(r.sba, k, lo, hi, bits)
            np.testing.assert_array_equal(h.astype(np.int64), want, err_msg=f"{tag} {r.label}: histogram of [{lo}, {hi})")
            if mixed:
                h = h.astype(np.uint64)
                rest, runs = eng.shard_class_b(lo, hi, k, h)
                want_rest, want_homo = class_b_starts(r.sba, r.seg, k, lo, hi)
                np.testing.assert_array_equal(rest, want_rest, err_msg=f"{tag} {r.label}: class B of [{lo}, {hi})")
                homo = [np.arange(f, f + c, dtype=np.int64) for f, c, _ in runs.tolist()]
                np.testing.assert_array_equal(np.concatenate(homo) if homo else np.zeros(0, np.int64), want_homo,
                                              err_msg=f"{tag} {r.label}: homopolymer runs of [{lo}, {hi})")
                added = int(h.astype(np.int64).sum()) - int(want.sum())
                assert added == len(rest) + sum((c * 11 + 15) // 16 for _, c, _ in runs.tolist()), (tag, r.label)
        # a world of 3 over position shares cut on the select's tile edges where the array reaches them
        b1 = T_SELECT if L > T_SELECT + 32 else L // 64 * 32
        b2 = 2 * T_SELECT if L > 2 * T_SELECT else b1 + (L - b1) // 64 * 32
        bounds = [0, b1, b2, L]
        hist, rests, runs_l = np.zeros(1 << bits, dtype=np.uint64), [], []
        for rank in range(world):
            h, _ = eng.shard_histogram(bounds[rank], bounds[rank + 1], k)
            h = h.astype(np.uint64)
            if mixed:
                rest, runs = eng.shard_class_b(bounds[rank], bounds[rank + 1], k, h)
                rests.append(rest)
                runs_l.append(runs)
            hist += h
        cuts = D.split_buckets(hist.astype(np.int64), world)
        for fused in ("0", "1"):
            monkeypatch.setitem(_native.options, "GKM_RANGE_FUSED", fused)
            parts = []
            for rank in range(world):
                if mixed:
                    n = eng.shard_sort_range_b(k, cuts[rank], cuts[rank + 1], np.concatenate(rests),
                                               np.concatenate(runs_l).reshape(-1, 3))
                else:
                    n = eng.shard_sort_range(k, cuts[rank], cuts[rank + 1])
                parts.append(eng.copy_starts())
                assert len(parts[-1]) == n, (tag, r.label)
            np.testing.assert_array_equal(np.concatenate(parts), r.want,
                                          err_msg=f"{tag} {r.label}: ranks concatenated, GKM_RANGE_FUSED={fused}")
