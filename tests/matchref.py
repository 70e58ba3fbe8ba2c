"""Host reference of matching statistics (gk_match / Kmers.match_lengths), numpy only -- TEST
INFRASTRUCTURE ONLY (a helper module, not a conftest).

Nothing here comes from the code under test.  From a host sba (ASCII bases, contigs joined by '$'),
min_kmer_len and max_kmer_len (None: whole suffixes up to '$'): the indexed k-mers are the strings
that start where min_kmer_len bytes hold no '$', cut at max_kmer_len bytes or at the '$'.  Only their
first C bytes (C = the cap) bear on a match of at most C, so the index is the rows of those bytes,
NUL after the k-mer's end: viewed as ``S{C}`` they compare in byte order with a shorter k-mer below
every extension of it, which is the reference comparator's order (compare_sba_kmers_lexicographically,
kmers.py:306-397: a k-mer that meets its contig's end first compares less).

``match_len`` comes from sets of prefixes: for every length l the distinct l-byte prefixes of the
k-mers that have l bytes; the length at a read position is the largest l, inside the read and at most
C, whose l bytes are in the set of l.  ``first`` and ``count`` come from bisection on the sorted rows:
the rows below the l bytes, and the rows up to the l bytes followed by 0xFF.  tests/test_matchref.py
pins all of it to a pure-Python brute force before any GPU test relies on it.
"""

import numpy as np

DOLLAR = ord("$")


def as_sba(seqs) -> np.ndarray:
    """The sba of a sequence list [(name, str)] or of one str / bytes: contigs joined by '$'."""
    if isinstance(seqs, np.ndarray):
        return np.ascontiguousarray(seqs, dtype=np.uint8)
    if isinstance(seqs, (str, bytes)):
        seqs = [("s", seqs)]
    parts = [s.encode() if isinstance(s, str) else bytes(s) for _, s in seqs]
    return np.frombuffer(b"$".join(parts), dtype=np.uint8)


def pack(reads):
    """(uint8[total], int64 offsets[nseq + 1]) of a list of str / bytes."""
    parts = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum(np.array([len(p) for p in parts], dtype=np.int64), out=offsets[1:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), offsets


def _as_s(mat, width):
    """rows of a uint8 matrix [r, width] as one ``S{width}`` each"""
    if mat.shape[0] == 0:
        return np.empty(0, dtype=f"S{width}")
    return np.ascontiguousarray(mat).view(f"S{width}").ravel()


class Index:
    """The indexed k-mers of (sba, min_kmer_len, max_kmer_len) as far as a cap of C bytes sees them."""

    def __init__(self, sba, min_len: int, max_len, cap: int):
        sba = as_sba(sba)
        cap = int(cap)
        assert cap >= 1 and min_len >= 1 and (max_len is None or cap <= max_len)
        self.cap = cap
        padded = np.concatenate([sba, np.full(max(cap, min_len), DOLLAR, dtype=np.uint8)])
        dollars = np.concatenate([[0], np.cumsum(padded == DOLLAR)])
        p = np.arange(len(sba))
        starts = p[dollars[p + min_len] == dollars[p]]  # min_len bytes without '$' (the pad is '$')
        rows = np.lib.stride_tricks.sliding_window_view(padded, cap)[starts].copy()
        ended = np.maximum.accumulate(rows == DOLLAR, axis=1)
        rows[ended] = 0
        self.starts = starts
        self.rows = rows                                   # [n, cap], NUL from the k-mer's end on
        self.lens = cap - ended.sum(axis=1)                # bytes of each k-mer below the cap
        self.sorted = np.sort(_as_s(rows, cap))            # the sorted order, as far as the cap sees it
        self.n = len(starts)
        self._prefixes = {}

    def prefixes(self, l: int):
        """the distinct l-byte prefixes (``S{l}``, ascending) of the k-mers that have l bytes"""
        if l not in self._prefixes:
            self._prefixes[l] = np.unique(_as_s(self.rows[self.lens >= l][:, :l], l))
        return self._prefixes[l]


def _member(uniq, rows):
    if len(uniq) == 0 or len(rows) == 0:
        return np.zeros(len(rows), dtype=bool)
    pos = np.searchsorted(uniq, rows, side="left")
    hit = np.zeros(len(rows), dtype=bool)
    inb = pos < len(uniq)
    hit[inb] = uniq[pos[inb]] == rows[inb]
    return hit


def match(index: Index, reads, cap=None) -> dict:
    """The expected gk_match of ``reads`` (a list of str / bytes) at cap ``cap`` (default: the
    index's): per byte of the batch ``lengths`` (uint32), ``first`` (uint64), ``count`` (uint32);
    ``offsets`` (uint64); per read ``longest`` (uint32), ``longest_pos`` (uint32), ``sum_len`` (uint64)."""
    C = index.cap if cap is None else int(cap)
    assert 1 <= C <= index.cap
    arr, offsets = pack(reads)
    nseq, total = len(offsets) - 1, len(arr)
    read_of = np.repeat(np.arange(nseq), np.diff(offsets))
    room = offsets[read_of + 1] - np.arange(total)          # bytes to the read's end
    lengths = np.zeros(total, dtype=np.int64)
    for l in range(1, min(C, total) + 1):
        at = np.flatnonzero(room >= l)
        win = np.lib.stride_tricks.sliding_window_view(arr, l)[at]
        hit = _member(index.prefixes(l), _as_s(win, l))
        lengths[at[hit]] = l                                 # (l ascends: the largest l that is present stays)
    first = np.zeros(total, dtype=np.int64)
    count = np.zeros(total, dtype=np.int64)
    W = index.cap
    for l in np.unique(lengths[lengths > 0]).tolist():
        at = np.flatnonzero(lengths == l)
        lo = np.zeros((len(at), W), dtype=np.uint8)
        lo[:, :l] = np.lib.stride_tricks.sliding_window_view(arr, l)[at]
        hi = lo.copy()
        hi[:, l:] = 0xFF
        a = np.searchsorted(index.sorted, _as_s(lo, W), side="left")
        b = np.searchsorted(index.sorted, _as_s(hi, W), side="right")
        first[at] = a
        count[at] = b - a
    longest = np.zeros(nseq, dtype=np.int64)
    longest_pos = np.zeros(nseq, dtype=np.int64)
    sum_len = np.zeros(nseq, dtype=np.int64)
    for j in range(nseq):
        v = lengths[offsets[j]:offsets[j + 1]]
        if len(v):
            longest[j] = v.max()
            longest_pos[j] = int(np.argmax(v)) if v.max() > 0 else 0  # (argmax: the first maximum)
            sum_len[j] = v.sum()
    return {
        "lengths": lengths.astype(np.uint32), "first": first.astype(np.uint64), "count": count.astype(np.uint32),
        "offsets": offsets.astype(np.uint64), "longest": longest.astype(np.uint32),
        "longest_pos": longest_pos.astype(np.uint32), "sum_len": sum_len.astype(np.uint64),
    }


def _common(a: bytes, b: bytes) -> int:
    t = 0
    while t < len(a) and t < len(b) and a[t] == b[t]:
        t += 1
    return t


PREV, NEXT = 1, 2


def neighbour_sides(index: Index, reads, cap=None) -> np.ndarray:
    """Per byte of the batch, which neighbour of the insertion point of the m bytes from there on (m =
    min(cap, bytes to the read's end)) shares the longest prefix with them: bit PREV the k-mer before,
    bit NEXT the k-mer at it; 0 where nothing matches.  For the tests' claims of coverage only."""
    C = index.cap if cap is None else int(cap)
    arr, offsets = pack(reads)
    srt = [bytes(s) for s in index.sorted.tolist()]
    out = np.zeros(len(arr), dtype=np.uint8)
    raw = arr.tobytes()
    import bisect
    for j in range(len(offsets) - 1):
        for p in range(int(offsets[j]), int(offsets[j + 1])):
            q = raw[p:min(p + C, int(offsets[j + 1]))]
            pos = bisect.bisect_left(srt, q)
            a = _common(srt[pos - 1], q) if pos > 0 else 0
            b = _common(srt[pos], q) if pos < len(srt) else 0
            if max(a, b) > 0:
                out[p] = (PREV if a >= b else 0) | (NEXT if b >= a else 0)
    return out


def maximal(lengths, offsets, min_len):
    """(read, pos, length) of the maximal matches, by a plain loop: position p of a read is reported
    iff lengths[p] >= min_len and (p is the read's first position or lengths[p - 1] < lengths[p] + 1)."""
    read, pos, length = [], [], []
    for j in range(len(offsets) - 1):
        a, b = int(offsets[j]), int(offsets[j + 1])
        for p in range(a, b):
            if lengths[p] >= min_len and (p == a or lengths[p - 1] < lengths[p] + 1):
                read.append(j)
                pos.append(p - a)
                length.append(int(lengths[p]))
    return np.array(read, dtype=np.int64), np.array(pos, dtype=np.int64), np.array(length, dtype=np.uint32)


def brute(seqs, min_len: int, max_len, reads, cap: int) -> dict:
    """The same answers as ``match`` in pure Python, for genomes of a few hundred bases: the k-mers as
    a sorted list of bytes, ``any(s.startswith(...))`` per length, counts by a scan."""
    if isinstance(seqs, (str, bytes)):
        seqs = [("s", seqs)]
    kmers = []
    for _, s in seqs:
        s = s.encode() if isinstance(s, str) else bytes(s)
        for p in range(len(s) - min_len + 1):
            kmers.append(s[p:] if max_len is None else s[p:p + max_len])
    kmers.sort()
    out = {k: [] for k in ("lengths", "first", "count")}
    per_read = {k: [] for k in ("longest", "longest_pos", "sum_len")}
    for r in reads:
        r = r.encode() if isinstance(r, str) else bytes(r)
        lens = []
        for p in range(len(r)):
            m = min(cap, len(r) - p)
            present = [any(s.startswith(r[p:p + l]) for s in kmers) for l in range(1, m + 1)]
            assert present == sorted(present, reverse=True)  # presence is monotone in l
            l = sum(present)
            lens.append(l)
            out["lengths"].append(l)
            q = r[p:p + l]
            out["first"].append(sum(1 for s in kmers if s[:l] < q and not s.startswith(q)) if l else 0)
            out["count"].append(sum(1 for s in kmers if s.startswith(q)) if l else 0)
        per_read["longest"].append(max(lens, default=0))
        per_read["longest_pos"].append(lens.index(max(lens)) if lens and max(lens) > 0 else 0)
        per_read["sum_len"].append(sum(lens))
    out.update(per_read)
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}
