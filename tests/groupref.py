"""Plain numpy reference of the group scan -- TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

Restates, from the behaviour the reference documents (mrperkett/genome-kmers v1.0.1, paths relative
to its src/genome_kmers/), the routines the device group pass replaces:

* ``filter_eval``  the six built-in filters (kmers.py:14-259; kmer_has_required_len kmers.py:262-282)
  for a whole start array at once, with the raise sites as gk_filter_error codes (include/gkm.h);
* ``group_scan``   kmer_info_by_group_generator (kmers.py:523-648) and get_kmer_group_size_hist
  (kmers.py:454-520) over the k-mers that pass, equality by compare_sba_kmers_lexicographically
  (kmers.py:306-397);
* ``first_raise``  the k-mer whose filter call raises first (the generator calls the filter in
  start-index order, kmers.py:579-596).

Unlike oracle/gk_oracle.c (one k-mer at a time) everything here is computed per position with
sliding windows -- prefix sums, run lengths, distance to the next '$' -- so 4.3 M positions take
seconds.  tests/test_groupref.py pins it against the golden vectors and the C oracle before any GPU
test relies on it.
"""

import numpy as np

DOLLAR = 36
_BIG = np.int64(1) << 60

KEEP_ALL, LENGTH, HOMOPOLYMER, GC, NO_AMBIGUOUS, CRISPR_NGG = range(6)
# gk_filter_error
FERR_HOMO_LEN, FERR_GC_LEN, FERR_GC_OOB, FERR_AMBIG_LEN, FERR_AMBIG_SEG, FERR_CRISPR_LEN = range(1, 7)
# the C oracle's names of the same raise sites (oracle.ERRORS)
ORACLE_ERROR_KIND = {FERR_HOMO_LEN: "homo_len", FERR_GC_LEN: "gc_len", FERR_GC_OOB: "gc_oob",
                     FERR_AMBIG_LEN: "ambig_len", FERR_AMBIG_SEG: "ambig_seg", FERR_CRISPR_LEN: "crispr_len"}


def _next_true(mask):
    """out[i] = the smallest j >= i with mask[j], _BIG if there is none; len(mask) + 1 entries."""
    n = len(mask)
    idx = np.where(mask, np.arange(n, dtype=np.int64), _BIG)
    out = np.empty(n + 1, dtype=np.int64)
    out[n] = _BIG
    out[:n] = np.minimum.accumulate(idx[::-1])[::-1]
    return out


def bases_before_end(sba):
    """out[p] = the number of bases from p up to the next '$' or the end of the sba; len + 1 entries."""
    sba = np.asarray(sba, dtype=np.uint8)
    nxt = np.minimum(_next_true(sba == DOLLAR), len(sba))
    return nxt - np.arange(len(sba) + 1, dtype=np.int64)


def _at(table, idx):
    """table[idx] with idx clamped to the table's last entry (its 'nothing found' sentinel)."""
    return table[np.minimum(idx, len(table) - 1)]


def filter_eval(sba, starts, kind, p0=0, p1=0, p2=0):
    """(passes bool[n], err_code int64[n]) of one built-in filter at every start; err_code is the
    gk_filter_error of the raise, 0 where the filter returns.  Within one k-mer the first event in
    the filter's own loop order decides (a homopolymer run that is too long returns False before a
    later '$' can raise, kmers.py:77-98; a G/C count above the maximum returns False before a later
    '$', kmers.py:165-188)."""
    sba = np.asarray(sba, dtype=np.uint8)
    s = np.asarray(starts, dtype=np.int64)
    L = len(sba)
    n = len(s)
    passes = np.zeros(n, dtype=bool)
    err = np.zeros(n, dtype=np.int64)
    p0, p1, p2 = int(p0), int(p1), int(p2)
    if kind == KEEP_ALL:
        passes[:] = True
    elif kind == LENGTH:  # kmers.py:19-34, 262-282
        passes[:] = bases_before_end(sba)[s] >= p0
    elif kind == HOMOPOLYMER:  # kmers.py:63-98
        maxh, k = p0, p1
        beyond = s + k - 1 >= L
        err[beyond] = FERR_HOMO_LEN
        short = ~beyond & (k < maxh)
        passes[short] = True
        scan = ~beyond & ~short
        # run[i] = length of the run of equal bytes that ends at i
        pos = np.arange(L, dtype=np.int64)
        first = np.ones(L, dtype=bool)
        first[1:] = sba[1:] != sba[:-1]
        run = pos - np.maximum.accumulate(np.where(first, pos, 0)) + 1
        # at offset t the loop has counted min(run[s + t], t + 1) equal bytes: above maxh first at
        # the first position >= s + maxh whose run is longer than maxh
        too_long = _at(_next_true(run > maxh), s + max(maxh, 1))
        dollar = _at(_next_true(sba == DOLLAR), s + 1)
        last = s + k - 1
        has_long = too_long <= last
        has_dollar = dollar <= last
        raises = scan & has_dollar & (~has_long | (dollar <= too_long))
        err[raises] = FERR_HOMO_LEN
        passes[scan & ~has_dollar & ~has_long] = True
    elif kind == GC:  # kmers.py:150-190
        minc, maxc, k = p0, p1, p2
        if maxc >= minc:
            is_gc = (sba == ord("G")) | (sba == ord("C"))
            cg = np.concatenate([[0], np.cumsum(is_gc)]).astype(np.int64)  # G/C in sba[:i]
            gc_pos = np.append(np.flatnonzero(is_gc), _BIG).astype(np.int64)
            # the position of the (maxc + 1)-th G/C at or after s: where the count passes maxc
            over = _at(gc_pos, cg[s] + max(maxc, 0))
            nd = bases_before_end(sba)[s]
            stop = s + nd  # the '$' or the end of the sba
            last = s + k - 1
            has_over = over <= last
            has_stop = stop <= last
            raises = has_stop & (~has_over | (stop < over))
            err[raises & (stop >= L)] = FERR_GC_OOB
            err[raises & (stop < L)] = FERR_GC_LEN
            whole = ~has_over & ~has_stop
            count = _at(cg, s + max(k, 0)) - cg[s]
            passes[whole] = (minc <= count[whole]) & (count[whole] <= maxc)
    elif kind == NO_AMBIGUOUS:  # kmers.py:209-227
        k = p0
        beyond = s + k > L
        err[beyond] = FERR_AMBIG_LEN
        acgt = (sba == ord("A")) | (sba == ord("C")) | (sba == ord("G")) | (sba == ord("T"))
        other = _at(_next_true(~acgt), s)
        hit = ~beyond & (other <= s + k - 1)
        is_dollar = np.zeros(n, dtype=bool)
        is_dollar[hit] = sba[other[hit]] == DOLLAR
        err[hit & is_dollar] = FERR_AMBIG_SEG
        passes[~beyond & ~hit] = True
    elif kind == CRISPR_NGG:  # kmers.py:232-259
        beyond = s + 23 > L
        err[beyond] = FERR_CRISPR_LEN
        ok = ~beyond
        passes[ok] = (sba[s[ok] + 21] == ord("G")) & (sba[s[ok] + 22] == ord("G"))
    else:
        raise ValueError(f"unknown filter kind {kind}")
    return passes, err


def first_raise(starts, err_code):
    """(sba index, gk_filter_error) of the first raise -- the lowest index of the current order with
    err_code != 0 -- or None if no k-mer raises."""
    bad = np.flatnonzero(np.asarray(err_code) != 0)
    if len(bad) == 0:
        return None
    return int(np.asarray(starts)[bad[0]]), int(err_code[bad[0]])


def _equal_to_previous(sba, s, kmer_len, chunk=1 << 20):
    """eq[q] (q >= 1) = k-mers s[q - 1] and s[q] compare equal at kmer_len (None: up to '$' / the
    end): the same effective length min(kmer_len, bases before '$' / end) and the same bytes over it
    (kmers.py:306-397 returns 0 exactly then).  Windows are compared column by column over the rows
    still undecided, about `chunk` rows at a time."""
    nd = bases_before_end(sba)[s]
    eff = nd if kmer_len is None else np.minimum(nd, int(kmer_len))
    eq = np.zeros(len(s), dtype=bool)
    for lo in range(1, len(s), chunk):
        hi = min(lo + chunk, len(s))
        a, b, la = s[lo - 1:hi - 1], s[lo:hi], eff[lo:hi]
        same = eff[lo - 1:hi - 1] == la
        rows = np.flatnonzero(same)
        t = 0
        while len(rows):
            rows = rows[la[rows] > t]
            differ = sba[a[rows] + t] != sba[b[rows] + t]
            same[rows[differ]] = False
            rows = rows[~differ]
            t += 1
        eq[lo:hi] = same
    return eq


def group_scan(sba, starts, kmer_len, valid=None, is_sorted=True, heads=None, min_group_size=1, max_group_size=None,
               yield_first_n=None, max_counts_bin=None):
    """The group scan over the k-mers with valid[i] (None: all), in the order given.

    Groups: runs of adjacent valid k-mers that compare equal at kmer_len (is_sorted); every valid
    k-mer its own group (is_sorted False, compare_sba_kmers_always_less_than kmers.py:295-303); or,
    with ``heads`` (GK_GROUPS_FROM_HEADS, include/gkm.h), a group starts at every valid position
    with heads[i] != 0 and at the first valid k-mer, heads at invalid positions being ignored.

    With max_counts_bin: (hist int64[max_counts_bin + 1], total) of the groups with min_group_size <=
    size <= max_group_size, sizes above the last bin counted in it (kmers.py:454-520).  Otherwise the
    generator's yields (kmers.py:523-648) as three arrays (kmer_num, group_size_yielded,
    group_size_total): the first yield_first_n members of every such group."""
    sba = np.asarray(sba, dtype=np.uint8)
    s = np.asarray(starts, dtype=np.int64)
    vidx = np.arange(len(s), dtype=np.int64) if valid is None else np.flatnonzero(np.asarray(valid)).astype(np.int64)
    cnt = len(vidx)
    if cnt:
        if heads is not None:
            head = np.asarray(heads)[vidx] != 0
        elif not is_sorted:
            head = np.ones(cnt, dtype=bool)
        else:
            head = ~_equal_to_previous(sba, s[vidx], kmer_len)
        head[0] = True
        gstart = np.flatnonzero(head)
        sizes = np.diff(np.append(gstart, cnt))
    else:
        gstart = sizes = np.zeros(0, dtype=np.int64)
    ok = sizes >= min_group_size
    if max_group_size is not None:
        ok &= sizes <= max_group_size
    if max_counts_bin is not None:
        hist = np.bincount(np.minimum(sizes[ok], max_counts_bin), minlength=max_counts_bin + 1).astype(np.int64)
        return hist, int(sizes[ok].sum())
    m = np.where(ok, sizes if yield_first_n is None else np.minimum(sizes, yield_first_n), 0)
    group = np.repeat(np.arange(len(sizes)), m)
    rank = np.arange(int(m.sum()), dtype=np.int64) - (np.cumsum(m) - m)[group]
    return (vidx[gstart[group] + rank].astype(np.uint64), m[group].astype(np.uint32),
            sizes[group].astype(np.uint32))


def scan_filtered(sba, starts, kmer_len, filt, **kw):
    """group_scan behind a built-in filter (kind, p0, p1, p2): ("raise", sba index, code) if a k-mer
    raises, else ("ok", result)."""
    passes, err = filter_eval(sba, starts, *filt)
    r = first_raise(starts, err)
    if r is not None:
        return ("raise",) + r
    return "ok", group_scan(sba, starts, kmer_len, valid=passes, **kw)


# ---------------------------------------------------------------------------------------------
# inputs shared by tests/test_groupref.py (vs the C oracle) and tests/test_gpu_groups.py (device)
# ---------------------------------------------------------------------------------------------
def segments_of(sba):
    return np.concatenate([[0], np.flatnonzero(np.asarray(sba) == DOLLAR) + 1]).astype(np.uint32)


def enumerate_starts(sba, min_kmer_len):
    """Every start with >= min_kmer_len bases before '$' / the end, ascending (kmers.py:789-861)."""
    sba = np.asarray(sba, dtype=np.uint8)
    nd = bases_before_end(sba)[:len(sba)]
    return np.flatnonzero((nd >= min_kmer_len) & (sba != DOLLAR)).astype(np.uint32)


def iupac_sequence(sba_len, contig_lens, seed, n_run=0):
    """An IUPAC sba of exactly sba_len bytes: contigs of contig_lens (the last takes what is left)
    joined by '$', a planted 900-base (or shorter) repeat rich in G/C and homopolymers, an N run
    of n_run bases in every contig long enough, and 'GG' as bases 3 and 4 of every contig after the
    first (crispr_ngg_pam_filter then passes a guide that crosses the '$')."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTNRY", dtype=np.uint8)
    lens = list(contig_lens)
    lens.append(sba_len - sum(lens) - len(lens))
    assert lens[-1] >= 1, "contig lengths leave no room for the last contig"
    rep = rng.choice(np.frombuffer(b"ACGTACGTGCCGGSAAAA", dtype=np.uint8), 900).astype(np.uint8)
    parts = []
    for L in lens:
        c = rng.choice(alphabet, L).astype(np.uint8)
        r = rep[:max(1, L // 5)]
        for _ in range(3):
            at = int(rng.integers(0, L - len(r) + 1))
            c[at:at + len(r)] = r
        if n_run and L > 4 * n_run:
            at = int(rng.integers(0, L - n_run))
            c[at:at + n_run] = ord("N")
        parts.append(c)
        parts.append(np.array([DOLLAR], dtype=np.uint8))
    sba = np.concatenate(parts[:-1])
    assert len(sba) == sba_len
    for d in np.flatnonzero(sba == DOLLAR):  # 'GG' where the guide that starts 18 before a '$' looks for its PAM
        sba[d + 3:d + 5] = ord("G")
    return sba


# (sba_len, contig lengths before the last, K = the enumeration's min_kmer_len, N-run length): the
# per-position filter pass packs 32 positions per word and one wave covers 64, so sba_len % 64 is 1
# and 33 at 2-4 scan tiles of k-mers (n % 16 != 0; one contig of exactly K bases), and 40 and 63 at
# less than one wave
EDGE_INPUTS = [(156 * 64 + 1, [4000, 31, 2500], 31, 300), (192 * 64 + 33, [5000, 3000], 31, 300),
               (40, [20], 8, 0), (63, [], 8, 0)]


def crispr_safe_starts(sba, starts):
    """starts without those whose 23-base guide + PAM would run past the end of the sba (where
    crispr_ngg_pam_filter raises, kmers.py:252-253); a guide that crosses a '$' in the middle of the
    sba is read across it and stays."""
    starts = np.asarray(starts)
    return starts[starts.astype(np.int64) + 23 <= len(sba)]


def filter_cases(K):
    """(label, (kind, p0, p1, p2)) for k-mers enumerated with min_kmer_len K: every built-in kind at
    ordinary parameters, at parameters that raise where a window of more than K bases meets a '$' or
    the end of the sba, and at the parameter edges of the filters."""
    third = K // 3
    lo, hi = int(np.ceil(K * 0.35)), int(np.floor(K * 0.6))
    lo5, hi5 = int(np.ceil((K + 5) * 0.3)), int(np.floor((K + 5) * 0.7))
    return [
        ("length-K", (LENGTH, K, 0, 0)),
        ("length-1-all-pass", (LENGTH, 1, 0, 0)),
        ("length-K+9", (LENGTH, K + 9, 0, 0)),
        ("homopolymer-3", (HOMOPOLYMER, 3, K, 0)),
        ("homopolymer-1", (HOMOPOLYMER, 1, K, 0)),
        ("homopolymer-raises", (HOMOPOLYMER, 4, K + 9, 0)),
        ("homopolymer-len-below-max", (HOMOPOLYMER, K + 4, K, 0)),          # kmer_len < max: all pass
        ("homopolymer-len-equals-max", (HOMOPOLYMER, K, K, 0)),             # the loop runs, no run can be too long
        ("homopolymer-len-below-max-past-end", (HOMOPOLYMER, K + 20, K + 9, 0)),  # raises at the end of the sba only
        ("gc-window", (GC, lo, hi, K)),
        ("gc-raises", (GC, lo5, hi5, K + 5)),
        ("gc-empty-window", (GC, K // 2 + 1, K // 2, K + 5)),               # ceil > floor: False before any read
        ("gc-exact-count", (GC, third, third, K)),
        ("gc-exact-zero", (GC, 0, 0, K)),
        ("gc-exact-all", (GC, K, K, K)),
        ("gc-max-only", (GC, 0, third, K + 5)),                             # False (count) races the '$'
        ("no-ambiguous-K", (NO_AMBIGUOUS, K, 0, 0)),
        ("no-ambiguous-raises", (NO_AMBIGUOUS, K + 2, 0, 0)),
        ("crispr-ngg", (CRISPR_NGG, 0, 0, 0)),
    ]
