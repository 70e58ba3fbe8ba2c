"""Plain numpy reference of the LCP array of a sorted k-mer order and what is read off it -- TEST
INFRASTRUCTURE ONLY (a helper module, not a conftest).

Works from the host sba and the sorted start indices alone and never calls the code under test.
``lcp[q]`` (q >= 1) is the largest k in 0..cap at which k-mers q - 1 and q compare equal under the
reference's compare_sba_kmers_lexicographically (mrperkett/genome-kmers v1.0.1,
src/genome_kmers/kmers.py:306-397) at kmer_len = k: the two windows are walked byte by byte; a '$' (or
the end of the sba) on both sides at the same offset means equal at every length (cap), on one side it
ends the common prefix, as a differing byte does.  ``lcp[0] = 0``, and ``lcp[n] = 0`` where a successor
is needed.  tests/test_lcpref.py pins all of it to tests/groupref.py (itself pinned to the C oracle and
the golden vectors) before any GPU test relies on it.
"""

import numpy as np

DOLLAR = 36
NEVER_UNIQUE = 0xFFFFFFFF


def lcp(sba, starts, cap, chunk=1 << 20):
    """uint32[n]: the common prefix, at most cap, of every k-mer of ``starts`` with its predecessor.
    The windows are compared column by column over the pairs still undecided, about ``chunk`` pairs
    at a time."""
    cap = int(cap)
    assert cap >= 1
    sp = np.append(np.asarray(sba, dtype=np.uint8), np.uint8(DOLLAR))  # the end of the sba reads as '$'
    s = np.asarray(starts, dtype=np.int64)
    out = np.zeros(len(s), dtype=np.uint32)
    for lo in range(1, len(s), chunk):
        hi = min(lo + chunk, len(s))
        a, b = s[lo - 1:hi - 1], s[lo:hi]
        res = np.full(hi - lo, cap, dtype=np.uint32)  # undecided at cap: equal at every length asked for
        rows = np.arange(hi - lo)
        t = 0
        while len(rows) and t < cap:
            x, y = sp[a[rows] + t], sp[b[rows] + t]
            end_a, end_b = x == DOLLAR, y == DOLLAR
            go_on = ~end_a & ~end_b & (x == y)
            stop = ~go_on & ~(end_a & end_b)  # a '$' on one side, or two different bases
            res[rows[stop]] = t
            rows = rows[go_on]
            t += 1
        out[lo:hi] = res
    return out


def pair_max(lcp_arr):
    """max(lcp[q], lcp[q + 1]) with lcp[n] = 0: the longest prefix k-mer q shares with a neighbour."""
    v = np.asarray(lcp_arr, dtype=np.int64)
    return np.maximum(v, np.append(v[1:], 0))


def spectrum(lcp_arr, cap):
    """(distinct int64[cap + 1], unique int64[cap + 1]): distinct[k] = #{q : lcp[q] < k},
    unique[k] = #{q : max(lcp[q], lcp[q + 1]) < k} for k = 1..cap; entry 0 is 0.  lcp_arr may have
    been computed at any cap >= this one."""
    cap = int(cap)
    v = np.minimum(np.asarray(lcp_arr, dtype=np.int64), cap)

    def below(values):
        counts = np.bincount(values, minlength=cap + 1)[:cap + 1]
        return np.concatenate([[0], np.cumsum(counts)[:cap]]).astype(np.int64)

    return below(v), below(pair_max(v))


def min_unique_track(sba_len, starts, lcp_arr, cap):
    """uint32[sba_len]: track[starts[q]] = max(lcp[q], lcp[q + 1]) + 1 if that is <= cap, else
    NEVER_UNIQUE; 0 where no k-mer starts."""
    m = pair_max(np.minimum(np.asarray(lcp_arr, dtype=np.int64), int(cap)))
    track = np.zeros(int(sba_len), dtype=np.uint32)
    track[np.asarray(starts, dtype=np.int64)] = np.where(m + 1 <= cap, m + 1, NEVER_UNIQUE).astype(np.uint32)
    return track


def group_sizes(heads):
    """per element, the size of the run it belongs to; runs start where heads is set (heads[0] is)"""
    heads = np.asarray(heads, dtype=bool)
    gstart = np.flatnonzero(heads)
    sizes = np.diff(np.append(gstart, len(heads)))
    return np.repeat(sizes, sizes)


def multiplicity_track(sba, starts, kmer_len, lcp_arr=None):
    """uint32[len(sba)]: track[starts[q]] = the size of q's group at kmer_len (None: whole k-mers up
    to '$'), groups being runs of a forward sorted order; 0 where no k-mer starts.  lcp_arr: the
    array of this order at a cap >= kmer_len, if the caller has it (else it is computed)."""
    s = np.asarray(starts, dtype=np.int64)
    track = np.zeros(len(sba), dtype=np.uint32)
    if len(s) == 0:
        return track
    k = len(sba) + 1 if kmer_len is None else int(kmer_len)
    heads = (lcp(sba, s, k) if lcp_arr is None else np.asarray(lcp_arr)) < k
    track[s] = group_sizes(heads)
    return track
