"""Host reference of the two-genome join (gk_join / Kmers.count_in / Kmers.compare), numpy only.

Nothing here comes from the code under test.  From a host sba (ASCII bases, contigs joined by '$'):
all K-byte windows that hold no '$' are the genome's k-mers; on canonical cases each is replaced by
the smaller of itself and its reverse complement (the complement table is spelt out below); the rows
viewed as ``S{K}`` compare in byte order, which is the reference comparator's order for whole k-mers
(compare_sba_kmers_lexicographically, kmers.py:306-397).  ``np.unique(..., return_counts=True)`` gives
the distinct k-mers and multiplicities of each side, ``np.searchsorted`` of A's distinct rows in B's
sorted rows gives ``b_first`` (gk_lookup's convention: the number of B's sorted k-mers that compare
less, the insertion point of an absent k-mer).
"""

import numpy as np

DOLLAR = ord("$")

# the reference's IUPAC complement (sequence_collection.py:402-433), spelt out
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B",
              "D": "H", "H": "D", "S": "S", "W": "W", "N": "N"}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in COMPLEMENT.items():
    COMP[ord(_a)] = ord(_b)

STAT_NAMES = ("n_distinct_a", "n_distinct_b", "n_shared", "occ_a_shared", "occ_b_shared", "occ_min")


def as_sba(seqs) -> np.ndarray:
    """The sba of a sequence list [(name, str)] or of one str / bytes: contigs joined by '$'."""
    if isinstance(seqs, np.ndarray):
        return np.ascontiguousarray(seqs, dtype=np.uint8)
    if isinstance(seqs, (str, bytes)):
        seqs = [("s", seqs)]
    parts = [s.encode() if isinstance(s, str) else bytes(s) for _, s in seqs]
    return np.frombuffer(b"$".join(parts), dtype=np.uint8)


def kmer_rows(sba, K: int, canonical: bool = False) -> np.ndarray:
    """``S{K}`` array of the genome's k-mers in position order (canonical forms if asked)."""
    sba = as_sba(sba)
    if len(sba) < K:
        return np.empty(0, dtype=f"S{K}")
    win = np.lib.stride_tricks.sliding_window_view(sba, K)
    win = np.ascontiguousarray(win[~(win == DOLLAR).any(axis=1)])
    rows = win.view(f"S{K}").ravel()
    if canonical:
        rc = np.ascontiguousarray(COMP[win][:, ::-1]).view(f"S{K}").ravel()
        rows = np.where(rc < rows, rc, rows)
    return rows


def join(sba_a, sba_b, K: int, canonical: bool = False) -> dict:
    """The expected join of genome A against genome B at length K:
    ``a_kmers`` (distinct, ascending) / ``a_count``, ``b_first`` (uint64) / ``b_count`` (uint32)
    aligned with them, ``b_kmers`` / ``b_mult`` (B's distinct k-mers), ``stats`` (the six sums)."""
    ra, rb = kmer_rows(sba_a, K, canonical), kmer_rows(sba_b, K, canonical)
    ua, ca = np.unique(ra, return_counts=True)
    ub, cb = np.unique(rb, return_counts=True)
    sorted_b = np.sort(rb)
    b_first = np.searchsorted(sorted_b, ua, side="left").astype(np.uint64)
    pos = np.searchsorted(ub, ua, side="left")
    hit = np.zeros(len(ua), dtype=bool)
    inb = pos < len(ub)
    hit[inb] = ub[pos[inb]] == ua[inb]
    b_count = np.zeros(len(ua), dtype=np.uint32)
    b_count[hit] = cb[pos[hit]]
    a_count = ca.astype(np.uint32)
    stats = {
        "n_distinct_a": len(ua), "n_distinct_b": len(ub), "n_shared": int(hit.sum()),
        "occ_a_shared": int(a_count[hit].sum(dtype=np.uint64)), "occ_b_shared": int(b_count.sum(dtype=np.uint64)),
        "occ_min": int(np.minimum(a_count, b_count).sum(dtype=np.uint64)),
    }
    return {"a_kmers": ua, "a_count": a_count, "b_first": b_first, "b_count": b_count, "b_kmers": ub,
            "b_mult": cb.astype(np.uint32), "stats": stats}


def derived(stats: dict) -> dict:
    """jaccard and containment as Kmers.compare documents them."""
    da, db, sh = stats["n_distinct_a"], stats["n_distinct_b"], stats["n_shared"]
    return {"jaccard": sh / (da + db - sh) if da + db - sh else 0.0, "containment": sh / da if da else 0.0}
