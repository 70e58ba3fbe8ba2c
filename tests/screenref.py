"""Host reference of the read screen (gk_screen / Kmers.screen), numpy only.

Nothing here comes from the code under test.  From a host sba (ASCII bases, contigs joined by '$'):
all K-byte windows that hold no '$' are the genome's k-mers; on canonical cases each is replaced by the
smaller of itself and its reverse complement (the complement table is spelt out below); the rows viewed
as ``S{K}`` compare in byte order, which is the reference comparator's order for whole k-mers
(compare_sba_kmers_lexicographically, kmers.py:306-397).  ``np.unique(..., return_counts=True)`` gives
the distinct k-mers and their multiplicities.  A batch of reads is cut the same way: every K-byte
window that lies inside one read is looked up among the distinct k-mers (its canonical form on
canonical cases; with ``both_strands`` on a forward case its reverse complement too, unless the window
is its own), which gives the count per byte position and, summed per read, the three per-read results.
"""

import numpy as np

DOLLAR = ord("$")

# the reference's IUPAC complement (sequence_collection.py:402-433), spelt out
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B",
              "D": "H", "H": "D", "S": "S", "W": "W", "N": "N"}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in COMPLEMENT.items():
    COMP[ord(_a)] = ord(_b)


def as_sba(seqs) -> np.ndarray:
    """The sba of a sequence list [(name, str)] or of one str / bytes: contigs joined by '$'."""
    if isinstance(seqs, np.ndarray):
        return np.ascontiguousarray(seqs, dtype=np.uint8)
    if isinstance(seqs, (str, bytes)):
        seqs = [("s", seqs)]
    parts = [s.encode() if isinstance(s, str) else bytes(s) for _, s in seqs]
    return np.frombuffer(b"$".join(parts), dtype=np.uint8)


def revcomp(s) -> str:
    """Reverse complement of a str / bytes, as a str."""
    b = s.encode() if isinstance(s, str) else bytes(s)
    return COMP[np.frombuffer(b, dtype=np.uint8)][::-1].tobytes().decode()


def _rows(win, K):
    return np.ascontiguousarray(win).view(f"S{K}").ravel()


def _rc_rows(win, K):
    return np.ascontiguousarray(COMP[win][:, ::-1]).view(f"S{K}").ravel()


def genome_kmers(sba, K: int, canonical: bool = False):
    """(distinct k-mers ``S{K}`` ascending, multiplicities) of the genome (canonical forms if asked)."""
    sba = as_sba(sba)
    if len(sba) < K:
        return np.empty(0, dtype=f"S{K}"), np.empty(0, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(sba, K)
    win = np.ascontiguousarray(win[~(win == DOLLAR).any(axis=1)])
    rows = _rows(win, K)
    if canonical:
        rc = _rc_rows(win, K)
        rows = np.where(rc < rows, rc, rows)
    return np.unique(rows, return_counts=True)


def pack(reads):
    """(uint8[total], int64 offsets[nseq + 1]) of a list of str / bytes."""
    parts = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum(np.array([len(p) for p in parts], dtype=np.int64), out=offsets[1:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), offsets


def _count_of(uniq, mult, rows):
    out = np.zeros(len(rows), dtype=np.int64)
    if len(uniq) == 0 or len(rows) == 0:
        return out
    pos = np.searchsorted(uniq, rows, side="left")
    inb = pos < len(uniq)
    hit = np.zeros(len(rows), dtype=bool)
    hit[inb] = uniq[pos[inb]] == rows[inb]
    out[hit] = mult[pos[hit]]
    return out


def screen(sba, K: int, reads, canonical: bool = False, both_strands: bool = False, index=None) -> dict:
    """The expected screen of ``reads`` (a list of str / bytes) against the genome at length K:
    ``window_counts`` (uint32 per byte of the batch: the count of the window starting there, 0 where
    none starts), ``offsets`` (uint64), and per read ``n_windows`` (uint32), ``n_present`` (uint32),
    ``occurrences`` (uint64).  ``index``: ``genome_kmers(sba, K, canonical)`` computed before, for
    callers that screen many batches against one genome."""
    uniq, mult = genome_kmers(sba, K, canonical) if index is None else index
    arr, offsets = pack(reads)
    nseq, total = len(offsets) - 1, len(arr)
    lens = np.diff(offsets)
    wc = np.zeros(total, dtype=np.int64)
    if total >= K:
        read_of = np.repeat(np.arange(nseq), lens)
        starts = np.arange(total - K + 1)
        inside = starts + K <= offsets[read_of[starts] + 1]
        win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(arr, K)[inside])
        rows = _rows(win, K)
        if canonical:
            rc = _rc_rows(win, K)
            cnt = _count_of(uniq, mult, np.where(rc < rows, rc, rows))
        else:
            cnt = _count_of(uniq, mult, rows)
            if both_strands:
                rc = _rc_rows(win, K)
                cnt = cnt + np.where(rc != rows, _count_of(uniq, mult, rc), 0)
        wc[starts[inside]] = cnt
    cum = np.concatenate([[0], np.cumsum(wc)])
    cump = np.concatenate([[0], np.cumsum(wc > 0)])
    return {
        "window_counts": wc.astype(np.uint32),
        "offsets": offsets.astype(np.uint64),
        "n_windows": np.maximum(lens - (K - 1), 0).astype(np.uint32),
        "n_present": (cump[offsets[1:]] - cump[offsets[:-1]]).astype(np.uint32),
        "occurrences": (cum[offsets[1:]] - cum[offsets[:-1]]).astype(np.uint64),
    }


def nontrivial(ref) -> bool:
    """Some windows present, some absent, some with a count above 1."""
    wc, nw = ref["window_counts"], int(ref["n_windows"].sum(dtype=np.int64))
    present = int((wc > 0).sum())
    return 0 < present < nw and bool((wc > 1).any())
