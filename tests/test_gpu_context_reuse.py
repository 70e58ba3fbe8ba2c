"""One context through every call that changes its k-mer set, and what must not survive the change.

A context caches views of its sorted order: the encoded keys, the group heads the MSD sort writes, the
unique view of gk_unique_counts and gk_lookup's prefix directory over the keys.  gk_set_sequence,
gk_enumerate, gk_set_start_indices and the shard sorts replace the set (set_kmer_set in
gkm_internal.h drops every view); a finished sort announces its keys (sort_finished).  Each case
below builds all the views on one engine, makes one such change, checks what the context answers
before it is sorted again, sorts, and compares starts, keys, 16 lookups and the unique view with a
fresh engine given the same calls -- a directory, head flags or a unique view left over from the
first sort would show as a difference.  Every comparison is exact.
"""

import numpy as np
import pytest

from genome_kmers import _native

pytestmark = pytest.mark.gpu

K = 12
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def two_contigs(seed, la, lb):
    """seeded A/C/G/T, two contigs; repeats inside and across them, so that the order has ties"""
    rng = np.random.default_rng(seed)
    a, b = ACGT[rng.integers(0, 4, la)], ACGT[rng.integers(0, 4, lb)]
    a[la // 2:la // 2 + 150] = a[100:250]
    b[lb // 3:lb // 3 + 90] = a[130:220]
    sba = np.concatenate([a, np.frombuffer(b"$", dtype=np.uint8), b])
    return np.ascontiguousarray(sba), np.array([0, la + 1], dtype=np.uint32)


SBA, SEG = two_contigs(20, 3000, 2000)
SBA2, SEG2 = two_contigs(21, 2500, 1700)  # (another sequence of another length)
N_KMERS = (3000 - K + 1) + (2000 - K + 1)


def make_queries():
    rng = np.random.default_rng(22)
    present = [bytes(SBA[i:i + K]) for i in (0, 100, 130, 1500, 2988, 3001, 3700, 4989)]
    absent = [bytes(ACGT[rng.integers(0, 4, K)]) for _ in range(8)]
    return _native.pack_queries(present + absent)


QUERIES = make_queries()


def snapshot(e):
    first, count = e.lookup(QUERIES)
    ustarts, ucounts = e.unique_counts()
    return {"starts": e.copy_starts(), "keys": e.copy_keys(), "first": first, "count": count,
            "unique_starts": ustarts, "unique_counts": ucounts}


def assert_same(got, want):
    assert got.keys() == want.keys()
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def loaded_engine():
    e = _native.Engine(0)
    e.set_sequence(SBA, SEG)
    return e


def base_state(monkeypatch):
    """sorted, the prefix directory built by a key-path lookup, the unique view built"""
    e = loaded_engine()
    e.enumerate(K)
    e.sort(K)
    with monkeypatch.context() as m:
        m.setitem(_native.options, "GKM_LOOKUP_PATH", "keys")  # (refused if the keys cannot serve it)
        e.profile_enable(True)
        first, count = e.lookup(QUERIES)
        stages = e.profile_report()
        e.profile_enable(False)
    assert stages["lookup_dir_build"]["count"] == 1 and stages["lookup_keys_dir"]["count"] == 1
    assert (count[:8] >= 1).all()
    e.unique_counts()
    return e


def expect_state_error(call, match):
    with pytest.raises(_native.GkError, match=match) as err:
        call()
    assert err.value.code == _native.GK_E_STATE


# each changer: (the change, the sort that follows it)
def change_sequence(e):
    e.set_sequence(SBA2, SEG2)


def sort_new_sequence(e):
    e.enumerate(K)
    e.sort(K)


def change_enumerate_longer(e):
    e.enumerate(K + 1)


def change_start_subset(e):
    # every K-mer start of the two contigs, and a shuffled half of them
    all_starts = np.concatenate([np.arange(0, 3000 - K + 1), np.arange(3001, 5001 - K + 1)]).astype(np.uint32)
    assert len(all_starts) == N_KMERS
    e.set_start_indices(np.random.default_rng(23).permutation(all_starts)[:N_KMERS // 2], K)


def change_shard_sort_range(e):
    _hist, bits = e.shard_histogram(0, len(SBA), K)
    assert e.shard_sort_range(K, 0, 1 << bits) == N_KMERS  # one rank owns every digit


CHANGERS = {
    "set_sequence": (change_sequence, sort_new_sequence),
    "enumerate_again": (lambda e: e.enumerate(K), lambda e: e.sort(K)),
    "enumerate_longer": (change_enumerate_longer, lambda e: e.sort(K + 1)),
    "set_start_indices": (change_start_subset, lambda e: e.sort(K)),
    "shard_sort_range": (change_shard_sort_range, lambda e: e.sort(K)),
}


@pytest.mark.parametrize("name", list(CHANGERS))
def test_views_do_not_survive_a_change_of_the_kmer_set(name, monkeypatch):
    change, sort_again = CHANGERS[name]
    e, fresh = base_state(monkeypatch), loaded_engine()
    change(e)
    change(fresh)
    if name == "shard_sort_range":  # the shard sort leaves a sorted set: its own keys, heads and directory
        assert e.key_layout() == fresh.key_layout() == (1, 2, K)
        assert_same(snapshot(e), snapshot(fresh))
    else:
        expect_state_error(e.key_layout, "no encoded keys")
        expect_state_error(lambda: e.lookup(QUERIES), "not sorted")
    sort_again(e)
    sort_again(fresh)
    assert e.key_layout() == fresh.key_layout()
    assert_same(snapshot(e), snapshot(fresh))


def test_plain_sort_after_quicksort_order(monkeypatch):
    """GK_SORT_QUICKSORT_ORDER moves members of tied groups only (keys, heads and the unique view
    stay); the plain sort behind it on the same context starts from those starts"""
    e, fresh = base_state(monkeypatch), loaded_engine()
    e.enumerate(K)  # (the quicksort's tie order depends on the order it starts from: the enumeration's)
    fresh.enumerate(K)
    e.sort(K, quicksort_order=True)
    fresh.sort(K, quicksort_order=True)
    got = snapshot(e)
    assert (got["unique_counts"] > 1).any(), "the set has no ties"
    assert_same(got, snapshot(fresh))
    e.sort(K)
    fresh.sort(K)
    plain = loaded_engine()
    plain.enumerate(K)
    plain.sort(K)
    want = snapshot(plain)
    assert (got["starts"] != want["starts"]).any(), "the quicksort order equals the plain one: nothing to undo"
    assert_same(snapshot(e), snapshot(fresh))
    assert_same(snapshot(e), want)
