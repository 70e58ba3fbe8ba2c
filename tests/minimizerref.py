"""NumPy reference of gk_minimizers / Kmers.minimizers (the definition: include/gkm.h).

``by_windows`` is the definition itself: enumerate the windows of w consecutive valid starts of one
sequence, take each window's leftmost position of least ord.  ``by_local_rule`` is the equivalent rule
per position (selected iff valid and L + R + 1 >= w), cheap enough for large inputs.  Both return
``(pos, ckey, strand, per_seq)``: batch byte positions ascending (uint64), canonical 2-bit keys (uint64),
strands (uint8) and the count per sequence (uint32).  ``mix`` in Python integers is the order hash."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MASK64 = (1 << 64) - 1
MIX_XOR = 0x9E3779B97F4A7C15


def fmix64(h: int) -> int:
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & MASK64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & MASK64
    h ^= h >> 33
    return h


def mix(x: int) -> int:
    return fmix64((x ^ MIX_XOR) & MASK64)


def mix_np(x: np.ndarray) -> np.ndarray:
    h = x.astype(np.uint64) ^ np.uint64(MIX_XOR)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _i


def as_batch(seqs):
    """(uint8 array, uint64 offsets) of a list of bytes / str, or of one."""
    if isinstance(seqs, (bytes, bytearray, str)):
        seqs = [seqs]
    parts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    arr = np.frombuffer(b"".join(parts), dtype=np.uint8)
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return arr, off


def revcomp_key(key: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (key & 3))
        key >>= 2
    return r


def position_keys(arr, off, k, canonical):
    """Per byte position: valid (bool), ckey (uint64), strand (uint8), seq (int64: its sequence)."""
    n = arr.size
    code = _CODE[arr]
    seq = np.searchsorted(off, np.arange(n, dtype=np.uint64), side="right").astype(np.int64) - 1
    end = off[seq + 1].astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    valid = (np.arange(n, dtype=np.int64) + k) <= end
    key = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    padded = np.concatenate([code, np.full(k, 4, dtype=np.uint8)])
    for t in range(k):
        c = padded[t:t + n]
        valid &= c < 4
        c2 = (c & 3).astype(np.uint64)
        key = (key << np.uint64(2)) | c2
        rc |= (np.uint64(3) - c2) << np.uint64(2 * t)
    strand = np.zeros(n, dtype=np.uint8)
    ckey = key
    if canonical:
        strand = (rc < key).astype(np.uint8)
        ckey = np.where(rc < key, rc, key)
    ckey = np.where(valid, ckey, np.uint64(0)).astype(np.uint64)
    strand = np.where(valid, strand, 0).astype(np.uint8)
    return valid, ckey, strand, seq


def _finish(sel, ckey, strand, off):
    pos = np.flatnonzero(sel).astype(np.uint64)
    lo = np.searchsorted(pos, off[:-1], side="left")
    hi = np.searchsorted(pos, off[1:], side="left")
    return pos, ckey[sel], strand[sel], (hi - lo).astype(np.uint32)


def ords_of(ckey, lex):
    return ckey.copy() if lex else mix_np(ckey)


def by_windows(arr, off, k, w, canonical=False, lex=False):
    """The definition: every window of w valid starts of one sequence selects its leftmost least ord."""
    arr = np.asarray(arr, dtype=np.uint8)
    off = np.asarray(off, dtype=np.uint64)
    valid, ckey, strand, _ = position_keys(arr, off, k, canonical)
    ord_ = ords_of(ckey, lex)
    sel = np.zeros(arr.size, dtype=bool)
    block = max(1, (1 << 21) // w)  # windows per slice of the view
    for j in range(off.size - 1):
        a, b = int(off[j]), int(off[j + 1])
        if b - a < w:
            continue
        nwin = b - a - w + 1
        for s0 in range(0, nwin, block):
            s1 = min(nwin, s0 + block)
            v = sliding_window_view(valid[a + s0:a + s1 + w - 1], w)
            o = sliding_window_view(ord_[a + s0:a + s1 + w - 1], w)
            exists = v.all(axis=1)
            arg = o.argmin(axis=1)  # (the first occurrence of the minimum: the leftmost)
            sel[a + s0 + np.flatnonzero(exists) + arg[exists]] = True
    return _finish(sel, ckey, strand, off)


def by_local_rule(arr, off, k, w, canonical=False, lex=False):
    """p is selected iff valid and L(p) + R(p) + 1 >= w (both capped at w - 1)."""
    arr = np.asarray(arr, dtype=np.uint8)
    off = np.asarray(off, dtype=np.uint64)
    n = arr.size
    valid, ckey, strand, seq = position_keys(arr, off, k, canonical)
    ord_ = ords_of(ckey, lex)
    L = np.zeros(n, dtype=np.int64)
    R = np.zeros(n, dtype=np.int64)
    alive_l = valid.copy()
    alive_r = valid.copy()
    for d in range(1, w):
        if d >= n or not (alive_l.any() or alive_r.any()):
            break
        nl = np.zeros(n, dtype=bool)  # position p - d continues L(p)
        nl[d:] = valid[:-d] & (seq[:-d] == seq[d:]) & (ord_[:-d] > ord_[d:])
        alive_l &= nl
        L += alive_l
        nr = np.zeros(n, dtype=bool)  # position p + d continues R(p)
        nr[:-d] = valid[d:] & (seq[d:] == seq[:-d]) & (ord_[d:] >= ord_[:-d])
        alive_r &= nr
        R += alive_r
    sel = valid & (L + R + 1 >= w)
    return _finish(sel, ckey, strand, off)
