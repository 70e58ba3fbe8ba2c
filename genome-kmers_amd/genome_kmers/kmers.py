"""Kmers -- drop-in for mrperkett/genome-kmers ``genome_kmers/kmers.py`` (v1.0.1) on MI355X.

The class surface (constructor, members, ``sort``, ``get_kmers``, ``get_kmer_count``,
``get_kmer_group_counts``, ``get_kmer_str``, the module-level comparators / filters / group
helpers) keeps the reference's names, argument meaning, error types and messages.  The work is
done by libgkm.so on the GPU (``_native.Engine``):

  enumerate   Kmers._initialize_single_pass (kmers.py:789-861)      -> gk_enumerate
  sort        Kmers.sort (kmers.py:1624-1731), numba quicksort        -> gk_sort (radix / doubling)
  groups      kmer_info_by_group_generator / get_kmer_group_size_hist
              (kmers.py:454-648) behind get_kmers / get_kmer_count /
              get_kmer_group_counts (kmers.py:869-1178)               -> gk_group_hist / gk_group_members

There is no CPU fallback for any of these.  Tie order: equal k-mers come out ordered by start
index -- the reference's ``get_is_less_than_func(break_ties=True)`` order (kmers.py:1710-1711).
The reference's default ``sort()`` leaves ties in numba-quicksort order, which no parallel sort
reproduces; sorted k-mers, group sizes and counts are identical either way.

The scalar helpers (``compare_sba_kmers_lexicographically``, the filter callables, ...) are kept
as host functions for API compatibility; when a built-in filter or comparator is handed to a
``Kmers`` method it is recognised and executed on the device instead.
"""

import shelve
from collections import namedtuple
from pathlib import Path
from typing import Callable, Generator, Union

import numpy as np

from . import _native
from .sequence_collection import SequenceCollection

DOLLAR = ord("$")
NEVER_UNIQUE = _native.NEVER_UNIQUE  # min_unique_lengths: not unique at any length up to max_len

# Kmers.screen's result: per read the number of windows, of windows present in the index and the sum of
# the windows' counts; with per_window=True also the count per byte position and the reads' offsets
ScreenResult = namedtuple("ScreenResult", ("n_windows", "n_present", "occurrences", "window_counts", "offsets"),
                          defaults=(None, None))
# Kmers.match_lengths' result: per read the longest match, the offset in the read of the first position
# that attains it and the sum of the positions' match lengths; with per_position=True also, per byte of
# the batch, the match length and its range of sorted positions, and the reads' offsets
MatchResult = namedtuple("MatchResult", ("longest", "longest_pos", "sum_len", "lengths", "first", "count", "offsets"),
                         defaults=(None, None, None, None))
MAX_MATCH_LEN = 4096  # the largest max_len of match_lengths when max_kmer_len is None
# Kmers.minimizers' result: read j's minimizers are entries offsets[j] .. offsets[j + 1] of pos (offset
# in the read), keys (the canonical 2-bit key) and strands (1: the key is the reverse complement's)
MinimizerResult = namedtuple("MinimizerResult", ("offsets", "pos", "keys", "strands"))
MAX_MINIMIZER_K = 32
MAX_MINIMIZER_W = 256


def maximal_from_lengths(lengths, offsets, min_len):
    """The maximal matches among per-position match lengths (``MatchResult.lengths`` and ``.offsets``):
    ``(read, pos, length)`` arrays (int64, int64, uint32) in batch order.  Position p of a read is
    reported iff ``lengths[p] >= min_len`` and p is the read's first position or
    ``lengths[p - 1] < lengths[p] + 1``: the match at p is not merely the tail of the match at p - 1.
    NumPy on the host, O(total bases)."""
    lengths = np.asarray(lengths)
    offsets = np.asarray(offsets).astype(np.int64)
    if lengths.ndim != 1 or offsets.ndim != 1 or offsets.size == 0 or int(offsets[-1]) != lengths.size:
        raise ValueError("maximal_from_lengths takes the per-position lengths and the reads' nseq + 1 offsets "
                         f"(lengths: {lengths.shape}, offsets: {offsets.shape})")
    v = lengths.astype(np.int64)
    keep = v >= int(min_len)
    if v.size:
        keep[1:] &= v[:-1] < v[1:] + 1
        first = offsets[:-1][offsets[:-1] < offsets[1:]]  # the first position of every non-empty read
        keep[first] = v[first] >= int(min_len)
    at = np.flatnonzero(keep)
    read = np.searchsorted(offsets, at, side="right") - 1
    return read.astype(np.int64), (at - offsets[read]).astype(np.int64), lengths[at].astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# filters (kmers.py:14-259): host-callable with the reference signature, plus a device spec
# ---------------------------------------------------------------------------------------------
class _DeviceFilter:
    """A built-in filter: callable as ``f(sba, sba_strand, kmer_sba_start_idx) -> bool`` and
    carrying the gk_filter record the device evaluates."""

    def __init__(self, kind: int, fn: Callable, p0: int = 0, p1: int = 0, p2: int = 0, kmer_len: int = None):
        self.kind = kind
        self._fn = fn
        self.params = (int(p0), int(p1), int(p2))
        self.kmer_len = kmer_len

    def __call__(self, sba, sba_strand, kmer_sba_start_idx):
        return self._fn(sba, sba_strand, kmer_sba_start_idx)

    def gk_filter(self) -> _native.GkFilter:
        return _native.GkFilter(self.kind, 0, *self.params)


class _JoinFilter:
    """Kmers.absent_from / Kmers.present_in: keep the k-mers of ``owner`` that are absent from /
    present in ``other``.  It has no host form: the device writes the mask from the join of the two
    sorted indexes (gk_join, gk_join_mask), so it serves ``get_kmers`` / ``get_kmer_count`` /
    ``get_kmer_group_counts`` of the Kmers that made it, at ``kmer_len == max_kmer_len``."""

    def __init__(self, owner: "Kmers", other: "Kmers", keep: int, name: str):
        self.owner = owner
        self.other = other
        self.keep = keep
        self.name = name

    def __call__(self, sba, sba_strand, kmer_sba_start_idx):
        raise TypeError(f"the filter of Kmers.{self.name} cannot be called as (sba, sba_strand, kmer_sba_start_idx): "
                        "it compares two sorted indexes on the device; pass it as kmer_filter_func to get_kmers, "
                        "get_kmer_count or get_kmer_group_counts of the Kmers that made it")

    def device_spec(self, engine: "_native.Engine", owner, kmer_len) -> _native.GkFilter:
        if owner is None:
            raise ValueError(f"the filter of Kmers.{self.name} belongs to a Kmers object: the array-level functions "
                             "(get_kmer_group_size_hist, kmer_info_by_group_generator) cannot evaluate it")
        if owner is not self.owner:
            raise ValueError(f"the filter of Kmers.{self.name} was made by another Kmers object: a filter of "
                             "a.absent_from(b) / a.present_in(b) filters the k-mers of a only")
        if kmer_len != owner.max_kmer_len:
            raise ValueError(f"the filter of Kmers.{self.name} compares k-mers at max_kmer_len ({owner.max_kmer_len}) "
                             f"only (kmer_len = {kmer_len})")
        owner._join(self.other, self.name)
        engine.join_mask(self.keep)
        return _native.GkFilter(_native.FILTER_MASK, 0, 0, 0, 0)


def _keep_all(sba, sba_strand, kmer_sba_start_idx):
    return True


kmer_filter_keep_all = _DeviceFilter(_native.FILTER_KEEP_ALL, _keep_all)


def gen_kmer_length_filter_func(min_kmer_len: int) -> Callable:
    """Pass if the k-mer has min_kmer_len bases before '$' (kmers.py:19-34)."""

    def filt(sba, sba_strand, kmer_sba_start_idx):
        return kmer_has_required_len(sba, kmer_sba_start_idx, min_kmer_len)

    return _DeviceFilter(_native.FILTER_LENGTH, filt, min_kmer_len)


def gen_kmer_homopolymer_filter_func(max_homopolymer_size: int, kmer_len: int) -> Callable:
    """Pass if no homopolymer is longer than max_homopolymer_size (kmers.py:37-100)."""
    if max_homopolymer_size < 1:
        raise ValueError(f"max_homopolymer_size ({max_homopolymer_size}) must be >= 1")
    if kmer_len < 1:
        raise ValueError(f"kmer_len ({kmer_len}) must be >= 1")

    def filt(sba, sba_strand, kmer_sba_start_idx):
        if kmer_sba_start_idx + kmer_len - 1 >= len(sba):
            raise ValueError(
                f"The kmer_len ({kmer_len}) requested is too large for kmer_sba_start_idx ({kmer_sba_start_idx})"
            )
        if kmer_len < max_homopolymer_size:
            return True
        size = 1
        for k in range(1, kmer_len):
            i = kmer_sba_start_idx + k
            if sba[i] == DOLLAR:
                raise ValueError(
                    f"The kmer_len ({kmer_len}) requested is too large for kmer_sba_start_idx ({kmer_sba_start_idx})"
                )
            if sba[i] == sba[i - 1]:
                size += 1
                if size > max_homopolymer_size:
                    return False
            else:
                size = 1
        return True

    return _DeviceFilter(_native.FILTER_HOMOPOLYMER, filt, max_homopolymer_size, kmer_len, kmer_len=kmer_len)


def gen_kmer_gc_content_filter_func(min_allowed_gc_frac: float, max_allowed_gc_frac: float, kmer_len: int) -> Callable:
    """Pass if the GC fraction lies in [min, max] (kmers.py:103-192)."""
    if min_allowed_gc_frac > max_allowed_gc_frac:
        raise ValueError(
            f"min_allowed_gc_frac ({min_allowed_gc_frac}) must be <= max_allowed_gc_frac ({max_allowed_gc_frac})"
        )
    if min_allowed_gc_frac < 0.0 or min_allowed_gc_frac > 1.0:
        raise ValueError(f"min_allowed_gc_frac ({min_allowed_gc_frac}) must be in the range [0.0, 1.0]")
    if max_allowed_gc_frac < 0.0 or max_allowed_gc_frac > 1.0:
        raise ValueError(f"max_allowed_gc_frac ({max_allowed_gc_frac}) must be in the range [0.0, 1.0]")
    min_count = int(np.ceil(kmer_len * min_allowed_gc_frac))
    max_count = int(np.floor(kmer_len * max_allowed_gc_frac))

    def filt(sba, sba_strand, kmer_sba_start_idx):
        if max_count < min_count:
            return False
        gc = 0
        for k in range(kmer_len):
            base = sba[kmer_sba_start_idx + k]
            if base == DOLLAR:
                raise ValueError(
                    f"The kmer_len ({kmer_len}) requested is too larger for kmer_sba_start_idx ({kmer_sba_start_idx})"
                )
            if base == 71 or base == 67:
                gc += 1
                if gc > max_count:
                    return False
        return min_count <= gc <= max_count

    return _DeviceFilter(_native.FILTER_GC, filt, min_count, max_count, kmer_len, kmer_len=kmer_len)


def gen_no_ambiguous_bases_filter(kmer_len: int) -> Callable:
    """Pass if the k-mer holds only A, T, G, C (kmers.py:195-229)."""

    def no_ambiguous_bases_filter(sba, sba_strand, kmer_sba_start_idx):
        if kmer_sba_start_idx + kmer_len > len(sba):
            raise ValueError(f"kmer_len ({kmer_len}) is invalid. It extends beyond len(sba)")
        for k in range(kmer_len):
            base = sba[kmer_sba_start_idx + k]
            if base == 36:
                raise ValueError(f"end of segment was reached. kmer_len ({kmer_len}) invalid.")
            if base not in (65, 84, 71, 67):
                return False
        return True

    return _DeviceFilter(_native.FILTER_NO_AMBIGUOUS, no_ambiguous_bases_filter, kmer_len, kmer_len=kmer_len)


def _crispr_ngg(sba, sba_strand, kmer_sba_start_idx) -> bool:
    if kmer_sba_start_idx + 23 > len(sba):
        raise ValueError("The guide defined at this start index extends beyond the sba")
    return bool(sba[kmer_sba_start_idx + 21] == 71 and sba[kmer_sba_start_idx + 22] == 71)


crispr_ngg_pam_filter = _DeviceFilter(_native.FILTER_CRISPR_NGG, _crispr_ngg)


def kmer_has_required_len(sba: np.ndarray, sba_start_idx: int, min_kmer_len: int) -> bool:
    """True if min_kmer_len bases precede '$' / the end (kmers.py:262-282)."""
    for idx in range(sba_start_idx, sba_start_idx + min_kmer_len):
        if idx >= len(sba) or sba[idx] == DOLLAR:
            return False
    return True


# ---------------------------------------------------------------------------------------------
# comparators (kmers.py:285-397)
# ---------------------------------------------------------------------------------------------
def compare_sba_kmers_lexicographically(sba_a, sba_b, kmer_sba_start_idx_a, kmer_sba_start_idx_b,
                                        max_kmer_len: Union[int, None] = None) -> tuple:
    """Three-way compare of two k-mers by ASCII bytes; '$' / end of array is smaller than any base.

    Returns (comparison, last_kmer_index_compared); see kmers.py:306-397.
    """
    k = 0
    while True:
        ia = kmer_sba_start_idx_a + k
        ib = kmer_sba_start_idx_b + k
        oa = ia >= len(sba_a) or sba_a[ia] == DOLLAR
        ob = ib >= len(sba_b) or sba_b[ib] == DOLLAR
        if oa or ob:
            last = k - 1
            if last < 0:
                raise AssertionError("There were no valid kmer bases to compare")
            if oa and not ob:
                return -1, last
            if ob and not oa:
                return 1, last
            return 0, last
        if sba_a[ia] < sba_b[ib]:
            return -1, k
        if sba_a[ia] > sba_b[ib]:
            return 1, k
        if max_kmer_len is not None and k == max_kmer_len - 1:
            return 0, k
        k += 1


class _Comparator:
    """compare_sba_kmers_lexicographically bound to a kmer_len; recognised by the device path."""

    def __init__(self, kmer_len, always_less=False):
        self.kmer_len = kmer_len
        self.always_less = always_less

    def __call__(self, sba_a, sba_b, kmer_sba_start_idx_a, kmer_sba_start_idx_b, max_kmer_len=None):
        if self.always_less:
            return -1, 0
        return compare_sba_kmers_lexicographically(sba_a, sba_b, kmer_sba_start_idx_a, kmer_sba_start_idx_b,
                                                   max_kmer_len=self.kmer_len)


def get_compare_sba_kmers_func(kmer_len):
    """Comparator with max_kmer_len = kmer_len (kmers.py:285-292)."""
    return _Comparator(kmer_len)


compare_sba_kmers_always_less_than = _Comparator(None, always_less=True)


# ---------------------------------------------------------------------------------------------
# group helpers (kmers.py:400-648)
# ---------------------------------------------------------------------------------------------
def get_kmer_info_minimal(kmer_num, kmer_sba_start_indices, sba, kmer_len, group_size_yielded, group_size_total):
    """(kmer_num, group_size_yielded, group_size_total) -- kmers.py:400-425"""
    return kmer_num, group_size_yielded, group_size_total


def get_kmer_info_group_size_only(kmer_num, kmer_sba_start_indices, sba, kmer_len, group_size_yielded,
                                  group_size_total):
    """group_size_total -- kmers.py:428-451"""
    return group_size_total


def _check_group_args(min_group_size, max_group_size, yield_first_n):
    # kmers.py:565-573
    if min_group_size < 1:
        raise ValueError(f"min_group_size ({min_group_size}) must be >= 1")
    if max_group_size is not None and max_group_size < min_group_size:
        raise ValueError(
            f"if max_group_size ({max_group_size}) is specified, it must be >= min_group_size ({min_group_size})"
        )
    if yield_first_n is not None and yield_first_n < 1:
        raise ValueError(f"if yield_first_n ({yield_first_n}) is specified, it must be > 0")


def _filter_error(ferr: int, sba_idx: int, filt) -> Exception:
    """Rebuild the exception the reference's filter raises (kmers.py:66-69, 176-179, 212-221, 252-253)."""
    k = getattr(filt, "kmer_len", None)
    if ferr == _native.FERR_HOMO_LEN:
        return ValueError(f"The kmer_len ({k}) requested is too large for kmer_sba_start_idx ({sba_idx})")
    if ferr == _native.FERR_GC_LEN:
        return ValueError(f"The kmer_len ({k}) requested is too larger for kmer_sba_start_idx ({sba_idx})")
    if ferr == _native.FERR_GC_OOB:
        return IndexError(f"kmer at sba index {sba_idx} of length {k} extends beyond len(sba)")
    if ferr == _native.FERR_AMBIG_LEN:
        return ValueError(f"kmer_len ({k}) is invalid. It extends beyond len(sba)")
    if ferr == _native.FERR_AMBIG_SEG:
        return ValueError(f"end of segment was reached. kmer_len ({k}) invalid.")
    if ferr == _native.FERR_CRISPR_LEN:
        return ValueError("The guide defined at this start index extends beyond the sba")
    return RuntimeError(f"device filter error {ferr} at sba index {sba_idx}")


def _device_filter(engine: "_native.Engine", filt, sba, sba_strand, starts_fn, owner=None,
                   kmer_len=None) -> _native.GkFilter:
    """gk_filter for a built-in filter; a custom Python callable is evaluated once per k-mer on the
    host (it is user code) into a mask that the device consumes.  A filter of Kmers.absent_from /
    present_in (``owner``: the Kmers whose method is filtering, at ``kmer_len``) runs the join and has
    the device write the mask."""
    if isinstance(filt, _DeviceFilter):
        return filt.gk_filter()
    if isinstance(filt, _JoinFilter):
        return filt.device_spec(engine, owner, kmer_len)
    if not callable(filt):
        raise TypeError("kmer_filter_func must be callable")
    starts = starts_fn()
    mask = np.fromiter((bool(filt(sba, sba_strand, int(s))) for s in starts), dtype=np.uint8, count=len(starts))
    engine.set_filter_mask(mask)
    return _native.GkFilter(_native.FILTER_MASK, 0, 0, 0, 0)


def _comparator_mode(cmp) -> tuple:
    """(is_sorted, kmer_len) for a recognised comparator; (None, None) for a custom one."""
    if isinstance(cmp, _Comparator):
        return (not cmp.always_less), cmp.kmer_len
    if not callable(cmp):
        raise TypeError("kmer_comparison_func must be callable")
    return None, None


def _custom_groups(engine: "_native.Engine", cmp, filt, sba, sba_strand, starts) -> _native.GkFilter:
    """A custom ``kmer_comparison_func`` (user code: the device cannot run it) decides the groups on
    the host, as the reference's generator does (kmers.py:579-601): each k-mer that passes the
    filter is compared with the previous one that passed, ``comparison == 0`` meaning the same
    group.  The filter runs on the host too, so that filter and comparator are called in the
    reference's order and the first raise is the reference's.  The device then runs the group
    pass over the resulting head mask (gk_set_group_heads); returns the filter spec to pass."""
    starts = np.asarray(starts)
    keep_all = isinstance(filt, _DeviceFilter) and filt.kind == _native.FILTER_KEEP_ALL
    if not keep_all and not callable(filt):
        raise TypeError("kmer_filter_func must be callable")
    valid = np.ones(len(starts), dtype=np.uint8)
    heads = np.zeros(len(starts), dtype=np.uint8)
    prev = None
    for i, s in enumerate(starts.tolist()):
        if not keep_all and not filt(sba, sba_strand, s):
            valid[i] = 0
            continue
        if prev is not None:
            comparison, _ = cmp(sba, sba, prev, s)
            heads[i] = comparison != 0
        prev = s
    engine.set_group_heads(heads)
    if keep_all:
        return filt.gk_filter()
    engine.set_filter_mask(valid)
    return _native.GkFilter(_native.FILTER_MASK, 0, 0, 0, 0)


def _engine_for_arrays(sba: np.ndarray, kmer_start_indices: np.ndarray) -> "_native.Engine":
    sba = np.ascontiguousarray(sba, dtype=np.uint8)
    seg = np.concatenate([[0], np.flatnonzero(sba == DOLLAR) + 1]).astype(np.uint32)
    eng = _native.Engine()
    eng.set_sequence(sba, seg)
    eng.set_start_indices(np.asarray(kmer_start_indices, dtype=np.uint32), 1)
    return eng


def get_kmer_group_size_hist(sba, sba_strand, kmer_len, kmer_start_indices, kmer_comparison_func, kmer_filter_func,
                             min_group_size: int = 1, max_group_size: Union[int, None] = None,
                             max_counts_bin: int = 1000000) -> tuple:
    """Histogram of group sizes and total k-mer count (kmers.py:454-520), on the device."""
    if max_counts_bin <= 0:
        raise ValueError(f"max_counts_bin ({max_counts_bin}) must be >= 1")
    _check_group_args(min_group_size, max_group_size, 1)
    is_sorted, cmp_len = _comparator_mode(kmer_comparison_func)
    if len(kmer_start_indices) == 0:
        return np.zeros(max_counts_bin + 1, dtype=np.int64), 0
    eng = _engine_for_arrays(sba, kmer_start_indices)
    if is_sorted is None:  # custom comparator: groups decided on the host, counted on the device
        filt = _custom_groups(eng, kmer_comparison_func, kmer_filter_func, sba, sba_strand, kmer_start_indices)
        return eng.group_hist(_native.GROUPS_FROM_HEADS, None, filt, min_group_size, max_group_size, max_counts_bin)
    filt = _device_filter(eng, kmer_filter_func, sba, sba_strand, lambda: kmer_start_indices)
    try:
        return eng.group_hist(is_sorted, cmp_len, filt, min_group_size, max_group_size, max_counts_bin)
    except _native.FilterRaised as e:
        raise _filter_error(e.ferr, e.sba_idx, kmer_filter_func) from None


def kmer_info_by_group_generator(sba, sba_strand, kmer_len, kmer_start_indices, kmer_comparison_func,
                                 kmer_filter_func, kmer_info_func, min_group_size: int = 1,
                                 max_group_size: Union[int, None] = None,
                                 yield_first_n: Union[int, None] = None) -> Generator[tuple, None, None]:
    """Yield kmer_info_func(...) for the first yield_first_n members of every group whose size lies
    in [min_group_size, max_group_size] (kmers.py:523-648); groups are computed on the device."""
    _check_group_args(min_group_size, max_group_size, yield_first_n)
    is_sorted, cmp_len = _comparator_mode(kmer_comparison_func)
    if len(kmer_start_indices) == 0:
        return
    eng = _engine_for_arrays(sba, kmer_start_indices)
    if is_sorted is None:  # custom comparator: groups decided on the host, members on the device
        filt = _custom_groups(eng, kmer_comparison_func, kmer_filter_func, sba, sba_strand, kmer_start_indices)
        nums, yielded, totals = eng.group_members(_native.GROUPS_FROM_HEADS, None, filt, min_group_size,
                                                  max_group_size, yield_first_n)
    else:
        filt = _device_filter(eng, kmer_filter_func, sba, sba_strand, lambda: kmer_start_indices)
        try:
            nums, yielded, totals = eng.group_members(is_sorted, cmp_len, filt, min_group_size, max_group_size,
                                                      yield_first_n)
        except _native.FilterRaised as e:
            raise _filter_error(e.ferr, e.sba_idx, kmer_filter_func) from None
    for num, y, t in zip(nums.tolist(), yielded.tolist(), totals.tolist()):
        yield kmer_info_func(num, kmer_start_indices, sba, kmer_len, y, t)


# ---------------------------------------------------------------------------------------------
# Kmers
# ---------------------------------------------------------------------------------------------
_UNSORTED_GROUP_MSG = (
    "Returning group parameters is not supported when kmers has not been"
    " sorted. {name} ({value}) cannot be specified. Did you"
    " mean to run sort() before getting kmers?"
)


class Kmers:
    """Memory-efficient k-mer calculations on a genome, resident on one MI355X."""

    # fixed-length Kmers run the first pass of the forward sort while the sequence is transferred
    # (gk_sort_hint); False skips it (see _get_engine for its cost)
    sort_prefetch = True

    def __init__(self, seq_coll: Union[SequenceCollection, None] = None, min_kmer_len: int = 1,
                 max_kmer_len: Union[int, None] = None, source_strand: str = "forward",
                 track_strands_separately: bool = False, method: str = "single_pass") -> None:
        # kmers.py:688-713 (same order of checks, same messages)
        if track_strands_separately:
            raise NotImplementedError(
                f"This function has not been implemented for track_strands_separately = '{track_strands_separately}'"
            )
        if source_strand != "forward":
            raise NotImplementedError(f"This function has not been implemented for source_strand = '{source_strand}'")
        if source_strand not in ("forward", "reverse_complement", "both"):
            raise ValueError(f"source_strand ({source_strand}) not recognized")
        if source_strand != "both" and track_strands_separately:
            raise ValueError(
                f"track_strands_separately can only be true if source_strand is 'both', but it is '{source_strand}'"
            )
        if min_kmer_len < 1:
            raise ValueError(f"min_kmer_len ({min_kmer_len}) must be greater than zero")
        if max_kmer_len is not None:
            if max_kmer_len < 1:
                raise ValueError(f"max_kmer_len ({max_kmer_len}) must be greater than zero")
            if min_kmer_len is not None and max_kmer_len < min_kmer_len:
                raise ValueError(f"max_kmer_len ({max_kmer_len}) is less than min_kmer_len ({min_kmer_len})")

        self.min_kmer_len = min_kmer_len
        self.max_kmer_len = max_kmer_len
        self.kmer_source_strand = source_strand
        self.track_strands_separately = track_strands_separately
        self._is_initialized = False
        self._is_set = False
        self._is_sorted = False
        self._canonical = False       # sorted by canonical k-mer (sort(canonical=True); no reference counterpart)
        self._engine = None
        self._host_starts = None      # host view of the start indices (or a user-assigned array)
        self._host_valid = True       # _host_starts matches the device order
        self._device_stale = False    # a user-assigned array has not been uploaded yet
        self._minimizer_spec = None   # (w, canonical, order) while the k-mer set is select_minimizers'

        if seq_coll is None:
            return

        # kmers.py:730-754
        min_seq_len = None
        num_records = 0
        for _, b, e in seq_coll.iter_records():
            seq_length = e - b + 1
            if min_seq_len is None or seq_length < min_seq_len:
                min_seq_len = seq_length
            num_records += 1
        if num_records == 0:
            raise ValueError("sequence_collection is empty")
        if min_kmer_len is not None and min_kmer_len > min_seq_len:
            raise ValueError(f"min_kmer_len ({min_kmer_len}) must be <= the shortest sequence length ({min_seq_len})")
        if seq_coll.strands_loaded() != source_strand:
            raise ValueError(
                f"source_strand ({source_strand}) does not match sequence_collection loaded strand "
                f"({seq_coll.strands_loaded()})"
            )
        self.seq_coll = seq_coll
        self._initialize(method=method)

    # ---- initialisation (kmers.py:762-861) ---------------------------------------------------
    def _initialize(self, kmer_filters=[], method: str = "single_pass"):
        if kmer_filters != []:
            raise NotImplementedError("kmer_filters have not been implemented")
        if method == "double_pass":
            raise NotImplementedError(f"method '{method}' has not been implemented")
        elif method == "single_pass":
            self._initialize_single_pass(kmer_filters=kmer_filters)
        else:
            raise ValueError(f"method '{method}' not recognized")
        self._is_initialized = True

    def _initialize_single_pass(self, kmer_filters=[]):
        if kmer_filters != []:
            raise NotImplementedError("kmer_filters have not been implemented")
        num_kmers = self._get_unfiltered_kmer_count()
        if num_kmers > 2**32 - 1:
            raise NotImplementedError("the size of the required kmers array exceeds the limit set by a uint32")
        eng = self._get_engine()
        n = eng.enumerate(self.min_kmer_len)
        if n != num_kmers:
            raise AssertionError(f"logic error: last_filled_index ({n - 1}) != num_kmers - 1 ({num_kmers - 1})")
        self._host_starts = None
        self._host_valid = False
        self._device_stale = False
        self._minimizer_spec = None

    def _get_unfiltered_kmer_count(self) -> int:
        num_kmers = 0
        num_records = 0
        for _, b, e in self.seq_coll.iter_records():
            num_kmers += (e - b + 1) - self.min_kmer_len + 1
            num_records += 1
        if num_records == 0:
            raise ValueError("SequenceCollection does not have any records")
        return num_kmers

    def _get_engine(self) -> "_native.Engine":
        if self._engine is None:
            eng = _native.Engine()
            # a fixed k-mer length: the transfer also runs the first pass of sort(k) (gk_sort_hint).
            # That pass costs device memory for every position (~13 B) and its work at load time;
            # a canonical, reference-order or unsorted workflow drops it, so such callers can set
            # Kmers.sort_prefetch = False (class- or instance-wide) before the first device call
            if self.sort_prefetch and self.min_kmer_len is not None and self.min_kmer_len == self.max_kmer_len:
                eng.sort_hint(self.min_kmer_len)
            eng.set_sequence(self.seq_coll.forward_sba, self.seq_coll._forward_sba_seg_starts)
            self._engine = eng
        return self._engine

    # ---- start indices: device-resident, host view on demand ---------------------------------
    @property
    def kmer_sba_start_indices(self):
        if not self._host_valid and self._engine is not None:
            n = self._engine.n
            buf = self._host_starts
            if buf is None or buf.shape != (n,) or buf.dtype != np.uint32 or not buf.flags.c_contiguous:
                buf = np.empty(n, dtype=np.uint32)
            writeable = buf.flags.writeable
            buf.setflags(write=True)
            self._engine.copy_starts(buf)
            buf.setflags(write=writeable)
            self._host_starts = buf
            self._host_valid = True
        return self._host_starts

    @kmer_sba_start_indices.setter
    def kmer_sba_start_indices(self, value):
        self._canonical = False
        self._minimizer_spec = None
        self._host_starts = value
        self._host_valid = True
        self._device_stale = True

    def _sync_device(self):
        """Upload a user-assigned start array before device work."""
        if self._device_stale:
            if self._host_starts is None:
                raise TypeError("kmer_sba_start_indices is None")
            self._get_engine().set_start_indices(np.asarray(self._host_starts, dtype=np.uint32), self.min_kmer_len)
            self._device_stale = False
            if self._canonical and self._is_sorted:
                # a canonical order loaded from a file: the device re-derives its canonical sorted
                # state (the same order: equal canonical k-mers are in start order either way)
                self._engine.sort(self.max_kmer_len, canonical=True)
        if self._engine is None:
            raise TypeError("Kmers has no sequence collection / k-mers")

    def _after_device_reorder(self):
        """Keep the reference's in-place semantics for a host array the caller already holds."""
        buf = self._host_starts
        if buf is not None and isinstance(buf, np.ndarray) and buf.dtype == np.uint32 and buf.flags.writeable \
                and buf.flags.c_contiguous and buf.shape == (self._engine.n,):
            self._engine.copy_starts(buf)
            self._host_valid = True
        else:
            self._host_valid = False

    def __len__(self):
        if self._engine is not None and not self._device_stale:
            return self._engine.n
        return len(self.kmer_sba_start_indices)

    def __getitem__(self):
        pass

    def _num_kmers(self) -> int:
        return len(self)

    def _check_forward(self):
        if self.kmer_source_strand != "forward" or self.seq_coll.strands_loaded() != "forward":
            raise NotImplementedError(
                f"both kmer_source_strand ({self.kmer_source_strand}) and "
                "sequence_collection.strands_loaded() must be 'forward'"
            )

    def _check_canonical_len(self, kmer_len):
        if self._is_sorted and getattr(self, "_canonical", False) and kmer_len != self.max_kmer_len:
            raise ValueError(f"canonical k-mers are grouped at kmer_len == {self.max_kmer_len} only "
                             f"(kmer_len = {kmer_len})")

    def _check_unsorted_group_args(self, min_group_size, max_group_size, yield_first_n=None):
        if not self._is_sorted:
            if min_group_size != 1:
                raise ValueError(_UNSORTED_GROUP_MSG.format(name="min_group_size", value=min_group_size))
            if max_group_size is not None:
                raise ValueError(_UNSORTED_GROUP_MSG.format(name="max_group_size", value=max_group_size))
            if yield_first_n is not None:
                raise ValueError(_UNSORTED_GROUP_MSG.format(name="yield_first_n", value=yield_first_n))

    def _filter_spec(self, filt, kmer_len):
        return _device_filter(self._engine, filt, self.seq_coll.forward_sba, self.seq_coll.strands_loaded(),
                              lambda: self.kmer_sba_start_indices, owner=self, kmer_len=kmer_len)

    # ---- queries (kmers.py:869-1178) ---------------------------------------------------------
    def get_kmers(self, kmer_len: Union[int, None], one_based_seq_index: bool = False,
                  kmer_filter_func: Callable = kmer_filter_keep_all, kmer_info_to_yield: str = "minimum",
                  min_group_size: int = 1, max_group_size: Union[int, None] = None,
                  yield_first_n: Union[int, None] = None) -> Generator[tuple, None, None]:
        """Yield k-mer info for qualifying groups (kmers.py:869-992); groups computed on the GPU."""
        self._check_forward()
        if kmer_len is not None and kmer_len < 1:
            raise ValueError(f"kmer_len ({kmer_len}) must be > 0")
        self._check_unsorted_group_args(min_group_size, max_group_size, yield_first_n)
        self._check_canonical_len(kmer_len)
        if kmer_info_to_yield not in ("minimum", "full"):
            raise ValueError(f"kmer_info_to_yield ({kmer_info_to_yield}) not recognized")
        _check_group_args(min_group_size, max_group_size, yield_first_n)
        self._sync_device()
        if self._engine.n == 0:
            return
        filt = self._filter_spec(kmer_filter_func, kmer_len)
        try:
            nums, yielded, totals = self._engine.group_members(self._is_sorted, kmer_len, filt, min_group_size,
                                                               max_group_size, yield_first_n)
        except _native.FilterRaised as e:
            raise _filter_error(e.ferr, e.sba_idx, kmer_filter_func) from None
        if kmer_info_to_yield == "minimum":
            for t in zip(nums.tolist(), yielded.tolist(), totals.tolist()):
                yield t
            return
        yield from self._full_info(nums, yielded, totals, kmer_len, one_based_seq_index)

    def _locate_records(self, nums, one_based):
        """Start, record and position in the record of each kmer_num: the starts and their segments
        come from the device (gk_locate), the record arithmetic of get_kmer_info (kmers.py:1180-1264)
        is vectorised here.  Returns (sba_strand, sba, names, seg, start, segment end, seq_idx)."""
        sc = self.seq_coll
        sba_strand = sc._get_sba_strand_to_use(sc.strands_loaded())
        sba, seg_starts, names = sc._strand_arrays(sba_strand)
        sba_idx, seg = self._engine.locate(nums)
        starts64 = seg_starts.astype(np.int64)
        b = starts64[seg]
        e = np.where(seg == len(seg_starts) - 1, len(sba) - 1, starts64[np.minimum(seg + 1, len(seg_starts) - 1)] - 2)
        s64 = sba_idx.astype(np.int64)
        seq_idx = (s64 - b if sba_strand == "forward" else e - s64) + (1 if one_based else 0)
        return sba_strand, sba, tuple(names), seg, s64, e, seq_idx

    def _full_info(self, nums, yielded, totals, kmer_len, one_based):
        """get_kmer_info (kmers.py:1180-1264) for every yielded k-mer at once (_locate_records); a
        k-mer whose kmer_len runs past its segment raises at its turn, as the reference's generator
        does."""
        sba_strand, sba, names, seg, s64, e, seq_idx = self._locate_records(nums, one_based)
        strand_char = "+" if sba_strand == "forward" else "-"
        klen = (e - s64 + 1) if kmer_len is None else np.full(len(s64), kmer_len, dtype=np.int64)
        bad = (s64 > e) | ((s64 + klen - 1) > e)
        first_bad = int(np.argmax(bad)) if bad.any() else len(s64)
        num_l, y_l, t_l, seg_l, seq_l, k_l = (nums.tolist(), yielded.tolist(), totals.tolist(), seg.tolist(),
                                              seq_idx.tolist(), klen.tolist())
        for i in range(first_bad):
            yield (num_l[i], strand_char, names[seg_l[i]], seq_l[i], k_l[i], y_l[i], t_l[i])
        if first_bad < len(s64):  # the reference's own checks and messages for that k-mer
            info = self.generate_get_kmer_info_func(one_based)
            i = first_bad
            yield info(num_l[i], self._start_lookup(num_l[i]), sba, kmer_len, y_l[i], t_l[i])

    def _start_lookup(self, kmer_num):
        """A one-element start view for generate_get_kmer_info_func's checks."""

        class _One:
            def __len__(_self):
                return int(self._engine.n)

            def __getitem__(_self, k):
                return int(self._engine.locate(np.array([k], dtype=np.uint64))[0][0])

        return _One()

    def get_kmer_count(self, kmer_len: Union[int, None], kmer_filter_func: Callable = kmer_filter_keep_all,
                       min_group_size: int = 1, max_group_size: Union[int, None] = None) -> int:
        """Total k-mers in qualifying groups (kmers.py:994-1083), on the GPU."""
        self._check_forward()
        if kmer_len is not None and kmer_len < 1:
            raise ValueError(f"kmer_len ({kmer_len}) must be > 0")
        self._check_unsorted_group_args(min_group_size, max_group_size)
        self._check_canonical_len(kmer_len)
        _, total = self._group_hist(kmer_len, kmer_filter_func, min_group_size, max_group_size, 1000000)
        return total

    def get_kmer_group_counts(self, kmer_len: Union[int, None], kmer_filter_func: Callable = kmer_filter_keep_all,
                              min_group_size: int = 1, max_group_size: Union[int, None] = None,
                              max_counts_bin: int = 1000000) -> tuple:
        """Histogram of group sizes + total (kmers.py:1085-1178), on the GPU."""
        self._check_forward()
        if kmer_len is not None and kmer_len < 1:
            raise ValueError(f"kmer_len ({kmer_len}) must be > 0")
        self._check_unsorted_group_args(min_group_size, max_group_size)
        self._check_canonical_len(kmer_len)
        if not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling get_kmer_group_counts")
        return self._group_hist(kmer_len, kmer_filter_func, min_group_size, max_group_size, max_counts_bin)

    def _group_hist(self, kmer_len, kmer_filter_func, min_group_size, max_group_size, max_counts_bin):
        if max_counts_bin <= 0:
            raise ValueError(f"max_counts_bin ({max_counts_bin}) must be >= 1")
        _check_group_args(min_group_size, max_group_size, 1)
        self._sync_device()
        if self._engine.n == 0:
            return np.zeros(max_counts_bin + 1, dtype=np.int64), 0
        filt = self._filter_spec(kmer_filter_func, kmer_len)
        try:
            return self._engine.group_hist(self._is_sorted, kmer_len, filt, min_group_size, max_group_size,
                                           max_counts_bin)
        except _native.FilterRaised as e:
            raise _filter_error(e.ferr, e.sba_idx, kmer_filter_func) from None

    def get_unique_kmers(self) -> tuple:
        """(first sorted index, multiplicity) of every distinct k-mer at the sort length -- the
        unique/count output of the device pipeline (no reference counterpart beyond the groups)."""
        if not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling get_unique_kmers")
        self._sync_device()
        return self._engine.unique_counts()

    # ---- lookup (no reference counterpart: the reference offers no search) ---------------------
    def find(self, kmers):
        """Where the given k-mers sit in the sorted order, searched on the GPU (gk_lookup).

        ``kmers``: one ``str`` / ``bytes``, a sequence of them (one length q), or a 2-D uint8 array
        (_native.pack_queries).  Returns ``(first, count)``: sorted positions
        ``[first, first + count)`` hold the k-mers whose first q bases equal the query under the
        reference's comparison (kmers.py:306-397); ``first`` is the insertion point of an absent
        query.  Arrays (uint64, uint32), or two ints for a single ``str`` / ``bytes``.  q may be
        shorter than max_kmer_len (a prefix range); after sort(canonical=True) only
        q == max_kmer_len, and a query and its reverse complement give the same range."""
        self._check_forward()
        if not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling find")
        single = isinstance(kmers, (str, bytes, bytearray))
        q = _native.pack_queries(kmers)
        if q.shape[0]:
            qlen = q.shape[1]
            if self.max_kmer_len is not None and qlen > self.max_kmer_len:
                raise ValueError(f"the k-mers have {qlen} characters, more than max_kmer_len ({self.max_kmer_len})")
            self._check_canonical_len(qlen)
        self._sync_device()
        first, count = self._engine.lookup(q)
        if single:
            return int(first[0]), int(count[0])
        return first, count

    def count(self, kmer) -> int:
        """Number of occurrences of one k-mer (find)."""
        return int(self.find(kmer)[1])

    def __contains__(self, kmer) -> bool:
        return self.count(kmer) > 0

    def get_kmer_locations(self, kmer, one_based_seq_index: bool = False) -> list:
        """[(strand, record_name, seq_idx)] of every occurrence of one k-mer, in sorted (ascending
        start) order: the range from find, the positions from the device (gk_locate).  After
        sort(canonical=True) the strand is "-" where the occurrence is the query's canonical form
        read from the reverse strand (get_canonical_strands of the range), else "+"."""
        if not isinstance(kmer, (str, bytes, bytearray)):
            raise ValueError("get_kmer_locations takes one k-mer (str or bytes)")
        first, count = self.find(kmer)
        if count == 0:
            return []
        nums = np.arange(first, first + count, dtype=np.uint64)
        sba_strand, _, names, seg, _, _, seq_idx = self._locate_records(nums, one_based_seq_index)
        strand_char = "+" if sba_strand == "forward" else "-"
        if self._canonical:
            strands = ["-" if r else "+" for r in self._engine.strand_range(first, count).tolist()]
        else:
            strands = [strand_char] * count
        return [(st, names[sg], sq) for st, sg, sq in zip(strands, seg.tolist(), seq_idx.tolist())]

    # ---- search with mismatches (no reference counterpart) -------------------------------------
    def _near_queries(self, kmers, max_mismatches):
        self._check_forward()
        q = _native.pack_queries(kmers)
        if q.shape[0]:
            qlen = q.shape[1]
            if qlen > 32:
                raise ValueError(f"the k-mers have {qlen} characters, more than 32")
            if max_mismatches > qlen:
                raise ValueError(f"max_mismatches ({max_mismatches}) is greater than the k-mers' length ({qlen})")
        if max_mismatches < 0:
            raise ValueError(f"max_mismatches ({max_mismatches}) must be >= 0")
        self._sync_device()
        return q

    def count_near(self, kmers, max_mismatches: int, both_strands: bool = False) -> np.ndarray:
        """How many k-mers lie within ``max_mismatches`` substitutions of each given k-mer, by distance:
        a scan of every position of the current order on the GPU (gk_lookup_mismatch; no sort needed).

        ``kmers`` as in find (q <= 32 characters).  Returns uint64 ``[m, max_mismatches + 1]``
        (1-D for a single ``str`` / ``bytes``): entry d counts the positions whose first q bytes hold
        no '$' and differ from the query in exactly d places (plain byte inequality: 'N' matches
        only 'N').  ``both_strands``: the reverse complement of the query is compared too, and a
        position counts once per strand on which it qualifies."""
        single = isinstance(kmers, (str, bytes, bytearray))
        q = self._near_queries(kmers, max_mismatches)
        counts = self._engine.mismatch_counts(q, max_mismatches, both_strands)
        return counts[0] if single else counts

    def find_near(self, kmers, max_mismatches: int, both_strands: bool = False, max_hits: int = 1 << 26) -> tuple:
        """The hits behind count_near: arrays ``(query, kmer_num, mismatches, strand)`` in ascending
        (query, kmer_num, strand).  ``kmer_num`` is the position in the order currently held (as in
        get_kmers); ``strand`` is 0 for the query as given, 1 for its reverse complement.  ValueError
        naming the total when there are more than ``max_hits`` hits."""
        q = self._near_queries(kmers, max_mismatches)
        return self._engine.mismatch_hits(q, max_mismatches, both_strands, max_hits)[1:]

    def get_near_locations(self, kmer, max_mismatches: int, both_strands: bool = False,
                           one_based_seq_index: bool = False) -> list:
        """[(strand, record_name, seq_idx, mismatches)] of every hit of one k-mer, in find_near's
        order; strand "-" where the reverse complement of the k-mer sits at that forward position."""
        if not isinstance(kmer, (str, bytes, bytearray)):
            raise ValueError("get_near_locations takes one k-mer (str or bytes)")
        _, nums, mism, strand = self.find_near(kmer, max_mismatches, both_strands)
        if len(nums) == 0:
            return []
        _, _, names, seg, _, _, seq_idx = self._locate_records(nums, one_based_seq_index)
        return [("-" if st else "+", names[sg], sq, mm)
                for st, sg, sq, mm in zip(strand.tolist(), seg.tolist(), seq_idx.tolist(), mism.tolist())]

    # ---- two genomes (no reference counterpart: the reference holds one genome at a time) ------
    def _join_checks(self, other, what):
        """The preconditions of gk_join, checked on the host before any device call."""
        if not isinstance(other, Kmers):
            raise ValueError(f"{what} compares two Kmers objects (self: Kmers, other: {type(other).__name__})")
        if not self._is_sorted or not other._is_sorted:
            raise AssertionError(f"The kmers must be sorted when calling {what} (self sorted: {self._is_sorted}, "
                                 f"other sorted: {other._is_sorted})")
        if self.kmer_source_strand != "forward" or other.kmer_source_strand != "forward":
            raise ValueError(f"{what} needs kmer_source_strand 'forward' on both sides (self: "
                             f"{self.kmer_source_strand!r}, other: {other.kmer_source_strand!r})")
        if self.max_kmer_len is None or self.max_kmer_len != other.max_kmer_len:
            raise ValueError(f"{what} needs one fixed max_kmer_len on both sides (self: {self.max_kmer_len}, "
                             f"other: {other.max_kmer_len})")
        for side, km in (("self", self), ("other", other)):
            if km.min_kmer_len != km.max_kmer_len:
                raise ValueError(f"{what} needs min_kmer_len == max_kmer_len, no k-mer cut short by a contig end "
                                 f"({side}: min_kmer_len = {km.min_kmer_len}, max_kmer_len = {km.max_kmer_len})")
        if self._canonical != other._canonical:
            raise ValueError(f"{what} needs both sides sorted the same way, canonical or not (self canonical: "
                             f"{self._canonical}, other canonical: {other._canonical})")

    def _join(self, other, what) -> dict:
        self._join_checks(other, what)
        self._sync_device()
        other._sync_device()
        return self._engine.join(other._engine)

    def count_in(self, other: "Kmers") -> tuple:
        """``(first, count)`` aligned with ``get_unique_kmers()``: for each distinct k-mer of this
        sorted index its multiplicity in ``other``'s and the number of ``other``'s sorted k-mers that
        compare less than it (its insertion point where the count is 0; find's convention), from
        one join of the two indexes on the GPU (gk_join).  Both sorted, one fixed length
        (min_kmer_len == max_kmer_len, the same on both sides), both canonical or neither."""
        self._join(other, "count_in")
        return self._engine.join_result()

    def compare(self, other: "Kmers") -> dict:
        """Shared and private k-mers of two sorted indexes (gk_join): the six sums of gk_join_stats
        (``n_distinct_a``, ``n_distinct_b``, ``n_shared``, ``occ_a_shared``, ``occ_b_shared``,
        ``occ_min``; a = self), ``jaccard`` = shared / (distinct in either; 0.0 when both are empty)
        and ``containment`` = shared / distinct in self."""
        st = self._join(other, "compare")
        da, db, shared = st["n_distinct_a"], st["n_distinct_b"], st["n_shared"]
        st["jaccard"] = shared / (da + db - shared) if da + db - shared else 0.0
        st["containment"] = shared / da if da else 0.0
        return st

    def absent_from(self, other: "Kmers") -> _JoinFilter:
        """A ``kmer_filter_func`` for this object's ``get_kmers`` / ``get_kmer_count`` /
        ``get_kmer_group_counts`` at ``kmer_len == max_kmer_len``: keep the k-mers that do not occur in
        ``other`` (the join runs when the filter is used, so it sees ``other`` as it is then)."""
        self._join_checks(other, "absent_from")
        return _JoinFilter(self, other, _native.JOIN_KEEP_ABSENT, "absent_from")

    def present_in(self, other: "Kmers") -> _JoinFilter:
        """As ``absent_from``, keeping the k-mers that occur in ``other``."""
        self._join_checks(other, "present_in")
        return _JoinFilter(self, other, _native.JOIN_KEEP_PRESENT, "present_in")

    # ---- reads against the index (no reference counterpart) -----------------------------------
    def screen(self, seqs, both_strands: bool = False, per_window: bool = False) -> ScreenResult:
        """How much of each read of a batch is in this sorted index, answered on the GPU (gk_screen).

        ``seqs``: one ``str`` / ``bytes`` (a batch of one), a list of them, or a packed
        ``(array, offsets)`` pair (_native.pack_sequences).  Every window of max_kmer_len bytes inside
        one read counts what ``find`` would return as ``count`` for it (after sort(canonical=True):
        for min(window, reverse complement)).  ``both_strands`` on a forward order adds the count of
        the window's reverse complement (once for a window that is its own); on a canonical order it
        changes nothing.  Returns ``ScreenResult``: per read ``n_windows`` (uint32, max(0, L - K + 1)),
        ``n_present`` (uint32, windows with a count above 0) and ``occurrences`` (uint64, the sum of
        the counts); with ``per_window`` also ``window_counts`` (uint32 per byte of the batch: the
        count of the window that starts there, 0 where none does) and the reads' ``offsets``."""
        self._check_forward()
        if not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling screen")
        if self.max_kmer_len is None:
            raise ValueError("screen needs a fixed max_kmer_len (the windows' length); max_kmer_len is None")
        arr, off = _native.pack_sequences(seqs)
        self._sync_device()
        n_present, occurrences, wc = self._engine.screen(arr, off, both_strands, per_window)
        lens = np.diff(off).astype(np.int64)
        n_windows = np.maximum(lens - (self.max_kmer_len - 1), 0).astype(np.uint32)
        if per_window:
            return ScreenResult(n_windows, n_present, occurrences, wc, off)
        return ScreenResult(n_windows, n_present, occurrences)

    # ---- minimizer sampling (no reference counterpart) -----------------------------------------
    @staticmethod
    def _minimizer_flags(what, k, w, canonical, order) -> int:
        if order not in ("hash", "lex"):
            raise ValueError(f"{what}: order must be 'hash' or 'lex' (order = {order!r})")
        if not 1 <= k <= MAX_MINIMIZER_K:
            raise ValueError(f"{what}: the k-mer length must be in 1..{MAX_MINIMIZER_K} (kmer_len = {k})")
        if not 1 <= w <= MAX_MINIMIZER_W:
            raise ValueError(f"{what}: w must be in 1..{MAX_MINIMIZER_W} (w = {w})")
        return (_native.MINIMIZER_CANONICAL if canonical else 0) | (_native.MINIMIZER_LEX if order == "lex" else 0)

    def minimizers(self, seqs, w: int, kmer_len: Union[int, None] = None, canonical: bool = False,
                   order: str = "hash") -> MinimizerResult:
        """The minimizers of every read of a batch, selected on the GPU (gk_minimizers).

        ``seqs`` as for ``screen`` (_native.pack_sequences).  A window is ``w`` consecutive k-mers of
        ``kmer_len`` bases (default: max_kmer_len, at most 32) made of A, C, G and T inside one read; its
        minimizer is its leftmost k-mer of least order -- a 64-bit hash of the 2-bit key
        (``order="hash"``) or the key itself (``"lex"``), with ``canonical`` of min(k-mer, reverse
        complement).  Returns ``MinimizerResult``: ``offsets`` (int64, nseq + 1) into ``pos`` (uint32,
        offset in the read, ascending per read), ``keys`` (uint64) and ``strands`` (uint8, 1 where the
        key is the reverse complement's).  Needs no sorted index."""
        if kmer_len is None:
            kmer_len = self.max_kmer_len
        if kmer_len is None:
            raise ValueError("minimizers needs kmer_len (max_kmer_len is None)")
        flags = self._minimizer_flags("minimizers", kmer_len, w, canonical, order)
        arr, off = _native.pack_sequences(seqs)
        # the batch needs no sequence: an object that has not uploaded its genome yet samples on a bare
        # context of its own (no upload, no sort-hint pass), never stored as the object's engine
        eng = self._engine
        if eng is None:
            eng = getattr(self, "_minimizer_engine", None)
            if eng is None:
                eng = self._minimizer_engine = _native.Engine()
        pos, keys, strands, per_seq = eng.minimizers((arr, off), kmer_len, w, flags)
        offsets = np.zeros(off.size, dtype=np.int64)
        np.cumsum(per_seq, out=offsets[1:])
        in_read = (pos - np.repeat(off[:-1], per_seq)).astype(np.uint32)
        return MinimizerResult(offsets, in_read, keys, strands)

    def select_minimizers(self, w: int, canonical: bool = False, order: str = "hash") -> int:
        """Replace the k-mer set by the genome's minimizers, selected on the GPU (gk_select_minimizers);
        returns their number.

        Needs min_kmer_len == max_kmer_len <= 32.  The selection is ``minimizers``' with the genome as
        one read ('$' and every letter but A, C, G, T end a run of windows), so a read that shares
        w + k - 1 bases with the genome picks the same k-mer there.  The object is unsorted afterwards
        and ``kmer_sba_start_indices`` reads the new set back on demand; ``sort``, ``find``,
        ``get_kmer_locations``, ``count_in`` and ``lcp`` then work as on any assigned start subset.
        (w, canonical, order) is remembered for ``find_minimizers`` until the start indices are assigned
        or the object is initialised again."""
        k = self.max_kmer_len
        if k is None or k != self.min_kmer_len or k > MAX_MINIMIZER_K:
            raise ValueError(f"select_minimizers needs min_kmer_len == max_kmer_len <= {MAX_MINIMIZER_K} "
                             f"(min_kmer_len = {self.min_kmer_len}, max_kmer_len = {self.max_kmer_len})")
        flags = self._minimizer_flags("select_minimizers", k, w, canonical, order)
        self._check_forward()
        n = self._get_engine().select_minimizers(k, w, flags)
        self._device_stale = False  # (an assigned array not yet uploaded is replaced too)
        self._host_starts = None
        self._host_valid = False
        self._is_sorted = False
        self._canonical = False
        self._minimizer_spec = (w, bool(canonical), order)
        return n

    def find_minimizers(self, seqs) -> tuple:
        """``(MinimizerResult, first, count)``: the reads' minimizers under the remembered
        select_minimizers spec, and ``find`` of each in this sorted sampled index.  The selected windows
        are gathered from the packed reads on the host (the lookup does not stay on the device)."""
        spec = getattr(self, "_minimizer_spec", None)
        if spec is None:
            raise ValueError("find_minimizers needs a k-mer set chosen by select_minimizers")
        w, canonical, order = spec
        if not self._is_sorted or self._canonical != canonical:
            raise ValueError(f"find_minimizers needs sort(canonical={canonical}) after "
                             f"select_minimizers(canonical={canonical})")
        arr, off = _native.pack_sequences(seqs)
        res = self.minimizers((arr, off), w, self.max_kmer_len, canonical, order)
        in_batch = res.pos.astype(np.int64) + np.repeat(off[:-1].astype(np.int64), np.diff(res.offsets))
        windows = arr[in_batch[:, None] + np.arange(self.max_kmer_len, dtype=np.int64)[None, :]]
        if windows.shape[0] == 0:
            return res, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
        first, count = self.find(np.ascontiguousarray(windows))
        return res, first, count

    # ---- matching statistics of reads (no reference counterpart) -------------------------------
    def _match_checks(self, what, max_len):
        """The preconditions of gk_match, checked on the host before any device call; returns the
        max_len to pass on (0: the sort length)."""
        if not self._is_sorted:
            raise AssertionError(f"The kmers must be sorted when calling {what}")
        if self.kmer_source_strand != "forward":
            raise ValueError(f"{what} needs kmer_source_strand 'forward' ({self.kmer_source_strand!r})")
        if getattr(self, "_canonical", False):
            raise ValueError(f"{what} needs a forward order: canonical k-mers have no prefixes (canonical: True)")
        if max_len is None:
            if self.max_kmer_len is None:
                raise ValueError(f"{what} needs max_len when max_kmer_len is None (the suffix order has no "
                                 f"length of its own; max_len: None)")
            return 0
        if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)):
            raise ValueError(f"max_len must be an int >= 1 (max_len: {max_len!r})")
        if max_len < 1:
            raise ValueError(f"max_len ({max_len}) must be >= 1")
        if self.max_kmer_len is not None and max_len > self.max_kmer_len:
            raise ValueError(f"max_len ({max_len}) is greater than max_kmer_len ({self.max_kmer_len})")
        if self.max_kmer_len is None and max_len > MAX_MATCH_LEN:
            raise ValueError(f"max_len ({max_len}) is greater than {MAX_MATCH_LEN}, the largest cap when "
                             f"max_kmer_len is None")
        return int(max_len)

    def match_lengths(self, seqs, max_len: Union[int, None] = None, per_position: bool = True) -> MatchResult:
        """How far each read matches the index from every position on: matching statistics, answered
        on the GPU (gk_match).

        ``seqs`` as in ``screen``.  For every byte position p of a read, ``lengths[p]`` is the length
        of the longest prefix of ``read[p:]`` -- at most ``max_len`` -- that ``find`` finds (count
        above 0), and ``first[p]``, ``count[p]`` are ``find``'s answer for that prefix (0, 0 where the
        length is 0).  A match never crosses the end of a read or of a contig.  ``max_len`` defaults
        to max_kmer_len and may not exceed it; when max_kmer_len is None it must be given, at most
        4096.  Returns ``MatchResult``: per read ``longest`` (uint32), ``longest_pos`` (uint32: the
        offset in the read of the first position that attains it) and ``sum_len`` (uint64); with
        ``per_position`` also ``lengths`` (uint32), ``first`` (uint64), ``count`` (uint32) per byte of
        the batch and the reads' ``offsets``.  Not available after sort(canonical=True); for the
        other strand pass the reverse-complemented reads."""
        cap = self._match_checks("match_lengths", max_len)
        arr, off = _native.pack_sequences(seqs)
        self._sync_device()
        longest, longest_pos, sum_len, lengths, first, count = self._engine.match(arr, off, cap, bool(per_position))
        if per_position:
            return MatchResult(longest, longest_pos, sum_len, lengths, first, count, off)
        return MatchResult(longest, longest_pos, sum_len)

    def maximal_matches(self, seqs, min_len: int, max_len: Union[int, None] = None) -> tuple:
        """The maximal exact matches of a batch of reads, at least ``min_len`` long: arrays
        ``(read, pos, length, first, count)`` -- the read, the offset in it, the match's length (capped
        at ``max_len`` as in ``match_lengths``) and its sorted positions ``[first, first + count)``,
        whose locations follow as for ``find`` (gk_locate).  A position is reported when its match is
        not merely the tail of the match one position before (maximal_from_lengths)."""
        if isinstance(min_len, bool) or not isinstance(min_len, (int, np.integer)) or min_len < 1:
            raise ValueError(f"min_len must be an int >= 1 (min_len: {min_len!r})")
        res = self.match_lengths(seqs, max_len, per_position=True)
        read, pos, length = maximal_from_lengths(res.lengths, res.offsets, min_len)
        at = res.offsets.astype(np.int64)[read] + pos
        return read, pos, length, res.first[at], res.count[at]

    # ---- the LCP array, the spectrum and the position tracks (no reference counterpart) ---------
    def _lcp_checks(self, what, length, name="max_len"):
        """The preconditions of gk_lcp / gk_lcp_spectrum / gk_position_track, checked on the host
        before any device call; returns the length to pass on (None resolved to max_kmer_len)."""
        if not self._is_sorted:
            raise AssertionError(f"The kmers must be sorted when calling {what}")
        if self.kmer_source_strand != "forward":
            raise ValueError(f"{what} needs kmer_source_strand 'forward' ({self.kmer_source_strand!r})")
        if length is None:
            if self.max_kmer_len is None:
                raise ValueError(f"{what} needs {name} when max_kmer_len is None (the suffix order has no "
                                 f"length of its own; {name}: None)")
            return self.max_kmer_len
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)):
            raise ValueError(f"{name} must be an int >= 1 ({name}: {length!r})")
        if length < 1:
            raise ValueError(f"{name} ({length}) must be >= 1")
        if self.max_kmer_len is not None and length > self.max_kmer_len:
            raise ValueError(f"{name} ({length}) is greater than max_kmer_len ({self.max_kmer_len})")
        return int(length)

    def lcp(self, max_len: Union[int, None] = None) -> np.ndarray:
        """The longest common prefix of every sorted k-mer with its predecessor (gk_lcp): uint32, in
        sorted order, ``lcp[0] == 0``.

        ``lcp[q]`` is the largest k in 0..``max_len`` at which k-mers q - 1 and q compare equal under
        the reference's comparison (kmers.py:306-397) at ``kmer_len = k``; two k-mers that end at a
        '$' after the same bases are equal at every length (``max_len``).  So the groups of
        ``get_kmer_group_counts(k)`` start where ``lcp < k``, for every k up to ``max_len`` at once.
        ``max_len`` defaults to max_kmer_len and may not exceed it.  When max_kmer_len is None (the
        suffix order) ``max_len`` must be given: inside long repeats the comparison costs up to
        ``max_len`` steps per pair of neighbours.  The array stays on the device as a view of the
        sorted order (a later call with a smaller ``max_len`` is served from it); not available
        after sort(canonical=True), where k-mers have no prefixes."""
        cap = self._lcp_checks("lcp", max_len)
        self._sync_device()
        return self._engine.lcp(cap)

    def kmer_spectrum(self, max_len: Union[int, None] = None) -> tuple:
        """``(distinct, unique)``: two int64 arrays indexed by k = 1..``max_len`` (entry 0 unused and 0),
        the number of distinct k-mers of length k and the number of those that occur once -- what
        ``get_kmer_group_counts(k)`` gives one k at a time -- from one pass over the LCP array
        (gk_lcp_spectrum).  ``max_len`` as in ``lcp``."""
        cap = self._lcp_checks("kmer_spectrum", max_len)
        self._sync_device()
        return self._engine.lcp_spectrum(cap)

    def min_unique_lengths(self, max_len: Union[int, None] = None) -> np.ndarray:
        """uint32[len(sba)] in sequence order: at the start of every k-mer the shortest length at which
        the k-mer that starts there occurs nowhere else, ``NEVER_UNIQUE`` where that is above
        ``max_len``, 0 where no k-mer of the current set starts ('$', contig tails shorter than
        min_kmer_len, positions outside assigned start indices).  ``max_len`` as in ``lcp``."""
        cap = self._lcp_checks("min_unique_lengths", max_len)
        self._sync_device()
        return self._engine.position_track(_native.TRACK_MIN_UNIQUE, cap, len(self.seq_coll.forward_sba))

    def multiplicity_track(self, kmer_len: Union[int, None] = None) -> np.ndarray:
        """uint32[len(sba)] in sequence order: at the start of every k-mer the number of k-mers equal
        to it at ``kmer_len`` (a mappability track), 0 where no k-mer of the current set starts.
        ``kmer_len`` defaults to max_kmer_len (None on a suffix order: whole suffixes up to '$');
        after sort(canonical=True) only max_kmer_len, where a k-mer and its reverse complement are
        one group."""
        if kmer_len is not None:
            kmer_len = self._lcp_checks("multiplicity_track", kmer_len, name="kmer_len")
        elif not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling multiplicity_track")
        self._sync_device()
        return self._engine.position_track(_native.TRACK_MULTIPLICITY, kmer_len or 0,
                                           len(self.seq_coll.forward_sba))

    def get_encoded_kmers(self) -> np.ndarray:
        """Encoded keys of the sorted k-mers, one row per k-mer."""
        if not self._is_sorted:
            raise AssertionError("The kmers must be sorted when calling get_encoded_kmers")
        return self._engine.copy_keys()

    def generate_get_kmer_info_func(self, one_based_seq_index: bool) -> Callable:
        """Location-rich info per yielded k-mer (kmers.py:1180-1264)."""
        get_record_info = self.seq_coll.generate_get_record_info_from_sba_index_func(one_based_seq_index)

        def get_kmer_info(kmer_num, kmer_sba_start_indices, sba, kmer_len, group_size_yielded, group_size_total):
            if kmer_num < 0:
                raise ValueError(f"kmer_num ({kmer_num}) cannot be less than zero")
            if kmer_num >= len(kmer_sba_start_indices):
                raise ValueError(
                    f"kmer_num ({kmer_num}) is out of bounds (num kmers = {len(kmer_sba_start_indices)})"
                )
            sba_idx = int(kmer_sba_start_indices[kmer_num])
            _, _, seg_end, seq_strand, seq_chrom, seq_start_idx = get_record_info(sba_idx)
            if kmer_len is None:
                kmer_len = seg_end - sba_idx + 1
            elif sba_idx + kmer_len - 1 > seg_end:
                raise ValueError(
                    f"kmer_len ({kmer_len}) for kmer_num ({kmer_num}) extends beyond the end of the segment"
                )
            return (kmer_num, seq_strand, seq_chrom, seq_start_idx, kmer_len, group_size_yielded, group_size_total)

        return get_kmer_info

    # ---- equality / persistence (kmers.py:1266-1531) -----------------------------------------
    def __ne__(self, other):
        return not self.__eq__(other)

    def __eq__(self, other):
        if self.min_kmer_len != other.min_kmer_len:
            return False
        if (self.max_kmer_len is None) != (other.max_kmer_len is None) or self.max_kmer_len != other.max_kmer_len:
            return False
        for attr in ("kmer_source_strand", "track_strands_separately", "_is_initialized", "_is_set", "_is_sorted"):
            if getattr(self, attr) != getattr(other, attr):
                return False
        a, b = self.kmer_sba_start_indices, other.kmer_sba_start_indices
        if (a is None) != (b is None):
            return False
        if a is not None and not np.array_equal(a, b):
            return False
        if getattr(self, "seq_coll", None) != getattr(other, "seq_coll", None):
            return False
        return True

    def save(self, save_file_path: Path, include_sequence_collection: bool = False, format: str = "hdf5",
             mode: str = "w") -> None:
        if format == "hdf5":
            self._save_hdf5(save_file_path, include_sequence_collection, mode=mode)
        elif format == "shelve":
            self._save_shelve(save_file_path, include_sequence_collection)
        else:
            raise ValueError(f"format ({format}) not recognized")

    def load(self, load_file_path: Path, seq_coll: Union[SequenceCollection, None] = None,
             format: str = "hdf5") -> None:
        if format == "hdf5":
            self._load_hdf5(load_file_path, seq_coll)
        elif format == "shelve":
            self._load_shelve(load_file_path, seq_coll)
        else:
            raise ValueError(f"format ({format}) not recognized")

    def _save_hdf5(self, save_file_path, include_sequence_collection=False, mode="w"):
        import h5py

        with h5py.File(save_file_path, mode) as f:
            g = f.create_group("kmers")
            g["min_kmer_len"] = self.min_kmer_len
            g["max_kmer_len"] = 0 if self.max_kmer_len is None else self.max_kmer_len
            g["kmer_source_strand"] = self.kmer_source_strand
            g["track_strands_separately"] = self.track_strands_separately
            g["_is_initialized"] = self._is_initialized
            g["_is_set"] = self._is_set
            # a canonical order is not the reference's sort order: the file says "not sorted" to the
            # reference's loader (kmers.py:939-960, 1435-1472), which then treats the object as
            # unsorted, and keeps the canonical state in keys of its own, which only this build reads
            g["_is_sorted"] = False if self._canonical else self._is_sorted
            s = self.kmer_sba_start_indices
            g["kmer_sba_start_indices"] = np.array([], dtype=np.uint32) if s is None else s
            if self._canonical:
                g["_canonical"] = True
                g["_canonical_sorted"] = bool(self._is_sorted)
        if include_sequence_collection:
            self.seq_coll.save(save_file_path, mode="a", format="hdf5")

    def _restore(self, starts, seq_coll, canonical=False):
        self.seq_coll = seq_coll
        self._engine = None
        if starts is not None and seq_coll is not None and seq_coll.forward_sba is not None:
            self.kmer_sba_start_indices = np.asarray(starts, dtype=np.uint32)
        else:
            self._host_starts = starts
            self._host_valid = True
            self._device_stale = starts is not None
            self._minimizer_spec = None
        # a canonical sort saved by this build (the reference has no canonical order); any other
        # file restores a forward order, whatever this object held before
        self._canonical = bool(canonical)

    def _load_hdf5(self, load_file_path, seq_coll=None):
        import h5py

        with h5py.File(load_file_path, "r") as f:
            g = f["kmers"]
            self.min_kmer_len = g["min_kmer_len"][()]
            mk = g["max_kmer_len"][()]
            self.max_kmer_len = None if mk == 0 else mk
            self.kmer_source_strand = g["kmer_source_strand"][()].decode("utf-8")
            self.track_strands_separately = g["track_strands_separately"][()]
            self._is_initialized = g["_is_initialized"][()]
            self._is_set = g["_is_set"][()]
            self._is_sorted = g["_is_sorted"][()]
            s = g["kmer_sba_start_indices"][:]
            starts = None if s.shape == (0,) else s
            canonical = bool(g["_canonical"][()]) if "_canonical" in g else False
            if canonical:
                # a canonical file written before the key existed: keep the stored flag
                if "_canonical_sorted" in g:
                    self._is_sorted = bool(g["_canonical_sorted"][()])
        if seq_coll is None:
            seq_coll = SequenceCollection()
            seq_coll.load(load_file_path, format="hdf5")
        self._restore(starts, seq_coll, canonical)

    def _save_shelve(self, save_file_path, include_sequence_collection=False):
        with shelve.open(str(save_file_path)) as db:
            for k in ("min_kmer_len", "max_kmer_len", "kmer_source_strand", "track_strands_separately",
                      "_is_initialized", "_is_set", "_is_sorted"):
                db[k] = getattr(self, k)
            db["kmer_sba_start_indices"] = self.kmer_sba_start_indices
            if self._canonical:  # as _save_hdf5: "not sorted" for the reference, canonical state apart
                db["_is_sorted"] = False
                db["_canonical"] = True
                db["_canonical_sorted"] = bool(self._is_sorted)
        if include_sequence_collection:
            self.seq_coll.save(save_file_path, format="shelve")

    def _load_shelve(self, load_file_path, seq_coll=None):
        with shelve.open(str(load_file_path)) as db:
            for k in ("min_kmer_len", "max_kmer_len", "kmer_source_strand", "track_strands_separately",
                      "_is_initialized", "_is_set", "_is_sorted"):
                setattr(self, k, db[k])
            starts = db["kmer_sba_start_indices"]
            canonical = bool(db.get("_canonical", False))
            if canonical:
                self._is_sorted = bool(db.get("_canonical_sorted", self._is_sorted))
        if seq_coll is None:
            seq_coll = SequenceCollection()
            seq_coll.load(load_file_path, format="shelve")
        self._restore(starts, seq_coll, canonical)

    # ---- readback (kmers.py:1533-1622) -------------------------------------------------------
    def _start_at(self, kmer_num: int) -> int:
        if self._host_valid and self._host_starts is not None:
            return int(self._host_starts[kmer_num])
        return int(self._engine.start_range(kmer_num, 1)[0])

    def get_kmer_str_no_checks(self, kmer_num: int, kmer_strand: str, kmer_len: int) -> str:
        if kmer_strand == "+":
            sba = self.seq_coll.forward_sba
            start = self._start_at(kmer_num)
        elif kmer_strand == "-":
            raise NotImplementedError("Only implemented for kmer_strand='+'")
        else:
            raise ValueError(f"kmer_strand ({kmer_strand}) not recognized")
        return bytes(sba[start : start + kmer_len]).decode("utf-8")

    def get_kmer_str(self, kmer_num: int, kmer_len: Union[int, None] = None) -> str:
        self._check_forward()
        if kmer_num < 0:
            raise ValueError(f"kmer_num ({kmer_num}) cannot be less than zero")
        if kmer_num >= len(self):
            raise ValueError(f"kmer_num ({kmer_num}) is out of bounds (num kmers = {len(self)})")
        if kmer_len is not None and kmer_len < self.min_kmer_len:
            raise ValueError(f"kmer_len ({kmer_len}) is less than min_kmer_len ({self.min_kmer_len})")
        if self.max_kmer_len is not None and kmer_len > self.max_kmer_len:  # TypeError for None, as kmers.py:1599
            raise ValueError(f"kmer_len ({kmer_len}) is greater than max_kmer_len ({self.max_kmer_len})")
        start = self._start_at(kmer_num)
        seg = self.seq_coll.get_segment_num_from_sba_index(start)
        _, seg_end = self.seq_coll.get_sba_start_end_indices_for_segment(seg)
        if kmer_len is None:
            largest = seg_end - start + 1
            kmer_len = largest if self.max_kmer_len is None else min(self.max_kmer_len, largest)
        if start + kmer_len - 1 > seg_end:
            raise ValueError(f"kmer_len ({kmer_len}) for kmer_num ({kmer_num}) extends beyond the end of the segment")
        return bytes(self.seq_coll.forward_sba[start : start + kmer_len]).decode("utf-8")

    # ---- sort (kmers.py:1624-1731) -----------------------------------------------------------
    def sort(self, *, canonical: bool = False, order: str = "stable"):
        """Sort the start indices by k-mer on the GPU (in place from the caller's point of view).

        Tie order (``order="stable"``, the default): equal k-mers come back in ascending start
        order -- the reference's ``get_is_less_than_func(break_ties=True)`` order
        (kmers.py:1710-1711).  The reference's own ``sort()`` uses ``break_ties=False`` and leaves
        equal k-mers in whatever order numba's quicksort produces (kmers.py:1624-1652); no parallel
        sort reproduces that.  ``order="reference"`` gives exactly that order: the device sorts,
        then numba's quicksort runs on the host over the original start order, comparing the
        device's group ranks (libgkm GK_SORT_QUICKSORT_ORDER; host-bound, 8 B of host memory per k-mer, not
        with canonical=True).  Sorted k-mers,
        encoded keys, group sizes, counts, histograms and the ``(kmer_num, group_size_yielded,
        group_size_total)`` tuples of ``get_kmers`` are identical either way, because ties only
        permute the members of a group inside the group's index range.  What can differ is WHICH
        members a tie group reports: the start (and so the location) behind a given ``kmer_num``
        inside a group, i.e. the members ``yield_first_n`` picks and the locations of
        ``kmer_info_to_yield="full"``.  Here they are the group's smallest start indices.

        canonical=True (this build's extension; the reference has no canonical k-mers,
        kmers.py:689-696): order by min(k-mer, reverse complement) with the reference's IUPAC
        complement (sequence_collection.py:402-433).  Needs min_kmer_len == max_kmer_len; groups,
        counts and encoded keys then refer to canonical k-mers (at kmer_len == max_kmer_len), and
        get_canonical_strands() tells which strand each sorted k-mer's canonical form came from.
        """
        self._check_forward()
        if order not in ("stable", "reference"):
            raise ValueError(f"order must be 'stable' or 'reference' (order = {order!r})")
        if canonical and order == "reference":
            raise ValueError("order='reference' is the reference's forward-strand quicksort order; the reference "
                             "has no canonical k-mers")
        if canonical and (self.max_kmer_len is None or self.max_kmer_len != self.min_kmer_len):
            raise ValueError(f"canonical k-mers need min_kmer_len == max_kmer_len (min_kmer_len = "
                             f"{self.min_kmer_len}, max_kmer_len = {self.max_kmer_len})")
        self._sync_device()
        try:
            self._engine.sort(self.max_kmer_len, canonical=canonical, quicksort_order=order == "reference")
        except _native.GkError as e:
            if e.code == _native.GK_E_NO_BASES:
                raise AssertionError(
                    f"kmers compared were less than min_kmer_len ({self.min_kmer_len}).  Was "
                    "kmer_sba_start_indices initialized correctly?"
                ) from None
            raise
        self._after_device_reorder()
        self._is_sorted = True
        self._canonical = canonical

    def get_canonical_strands(self) -> np.ndarray:
        """uint8 per sorted k-mer after sort(canonical=True): 1 if the canonical form is the k-mer's
        reverse complement (strictly smaller), 0 if it is the k-mer itself (or a palindrome)."""
        if not (self._is_sorted and self._canonical):
            raise AssertionError("get_canonical_strands needs sort(canonical=True)")
        return self._engine.copy_strands()

    def get_is_less_than_func(self, validate_kmers: bool = True, break_ties: bool = False) -> Callable:
        """Scalar is_less_than(a, b) of the reference (kmers.py:1654-1731), host-side, for callers
        that compare individual k-mers; Kmers.sort() does not use it."""
        self._check_forward()
        sba = self.seq_coll.forward_sba
        min_kmer_len, max_kmer_len = self.min_kmer_len, self.max_kmer_len

        def is_less_than(a: int, b: int) -> bool:
            comparison, last = compare_sba_kmers_lexicographically(sba, sba, a, b, max_kmer_len=max_kmer_len)
            if comparison < 0:
                lt = True
            elif comparison > 0:
                lt = False
            else:
                lt = (a < b) if break_ties else False
            if validate_kmers:
                nb = min_kmer_len - (last + 1)
                if not kmer_has_required_len(sba, a + last + 1, nb) or not kmer_has_required_len(sba, b + last + 1, nb):
                    raise AssertionError(
                        f"kmers compared were less than min_kmer_len ({min_kmer_len}).  Was "
                        "kmer_sba_start_indices initialized correctly?"
                    )
            return lt

        return is_less_than

    def to_csv(self, kmer_len, output_file_path, fields=["kmer"]):
        pass
