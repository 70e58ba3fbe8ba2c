#!/usr/bin/env python3
"""Speed of gk_lookup_mismatch at the ABI boundary (host arrays in, host arrays out), per path, against
the route that was available before it: the Hamming ball of every query through gk_lookup.

Genome: gk_reference_random_bases(--bases) cut into --contigs contigs, sorted once at --k.  Queries:
--k-mers sampled from the genome, query i with i % 5 planted substitutions (0..4).
Scan: one counts-only gk_lookup_mismatch call per (path keys | bytes, m, d, forward | both strands),
warm (one untimed call first), --repeats timed calls with the host clock around the call (the call
synchronises the stream); median, min, max, spread, and k-mer x query pairs per second of the median.
A pass of its own with gk_profile_enable gives the device time of the scan kernel alone.  A second
table times the two-call hits form (counts call, then hits call) on the key path.
Yardstick (m = --ball-queries, forward): every string within d substitutions of each query, generated
on the host (NOT timed, which favours this route), looked up in one gk_lookup call on the key path
with the prefix directory; the counts by distance are summed over each query's ball and must equal
the scan's counts.  The script asserts that, and that at d = 4 the scan's median is below the ball
route's median.

    python tools/mismatch_bench.py --out profiles/mismatch/mismatch_1e8.json
"""

import argparse
import ctypes
import itertools
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "genome-kmers_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from genome_kmers import _native  # noqa: E402
from lookup_bench import box_info, make_genome  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KERNEL_R = 4  # k-mers per thread of the scan kernel (kMismatchR, gkm_mismatch.hip)
COUNT_SCHEME = "64-bit global atomics behind a wave-uniform hit test; hit records appended once per wave"


def clear_knobs():
    for knob in ("GKM_MISMATCH_PATH", "GKM_LOOKUP_PATH", "GKM_LOOKUP_DIR"):
        if knob in _native.options:
            del _native.options[knob]


def make_queries(sba, k, m, seed):
    """windows of the genome without '$', query i with i % 5 substitutions at distinct places"""
    rng = np.random.default_rng(seed)
    out = np.empty((m, k), dtype=np.uint8)
    filled = 0
    while filled < m:
        s = rng.integers(0, len(sba) - k + 1, m - filled + 64)
        win = sba[s[:, None] + np.arange(k)[None, :]]
        win = win[(win != 36).all(axis=1)][: m - filled]
        out[filled:filled + len(win)] = win
        filled += len(win)
    code = np.searchsorted(ACGT, out)  # A C G T -> 0 1 2 3 (ASCII order)
    for i in range(m):
        pos = rng.choice(k, size=i % 5, replace=False)
        code[i, pos] = (code[i, pos] + rng.integers(1, 4, len(pos))) % 4
    return ACGT[code]


def ball_shell(queries, d):
    """every string at Hamming distance exactly d of each query: uint8 [m, C(k, d) 3^d, k]"""
    m, k = queries.shape
    code = np.searchsorted(ACGT, queries)
    if d == 0:
        return queries[:, None, :].copy()
    pos = np.array(list(itertools.combinations(range(k), d)), dtype=np.int64)  # [C, d]
    add = np.array(list(itertools.product((1, 2, 3), repeat=d)), dtype=np.int64)  # [S, d]
    C, S = len(pos), len(add)
    out = np.broadcast_to(code[:, None, None, :], (m, C, S, k)).astype(np.uint8)
    ci = np.arange(C)[:, None, None]
    si = np.arange(S)[None, :, None]
    for j in range(m):  # (one query at a time: the index arrays stay small)
        out[j, ci, si, pos[:, None, :]] = (code[j][pos][:, None, :] + add[None, :, :]) % 4
    return ACGT[out.reshape(m, C * S, k)]


def stats(ts, pairs=None):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    r = {"median_ms": med * 1e3, "min_ms": ts[0] * 1e3, "max_ms": ts[-1] * 1e3, "spread": (ts[-1] - ts[0]) / med}
    if pairs:
        r["pairs_per_s"] = pairs / med
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--m", default="100,1000")
    ap.add_argument("--d", default="1,2,3,4")
    ap.add_argument("--paths", default="keys,bytes")
    ap.add_argument("--ball-queries", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, k = int(args.bases), args.k
    ms = [int(x) for x in args.m.split(",")]
    ds = [int(x) for x in args.d.split(",")]
    paths = args.paths.split(",")
    assert _native.device_count() > 0, "mismatch_bench needs a GPU"
    assert args.ball_queries in ms and "keys" in paths, \
        "the yardstick compares with the key-path scan of the same batch: --m must hold --ball-queries, --paths keys"
    box = box_info()

    sba, seg = make_genome(bases, args.contigs, args.seed)
    queries = make_queries(sba, k, max(ms + [args.ball_queries]), args.seed + 1)
    e = _native.Engine()
    e.set_sequence(sba, seg)
    n = e.enumerate(k)
    e.sort(k)
    e.sync()
    P = ctypes.POINTER

    def scan(q, d, both, counts):
        total = ctypes.c_uint64(0)
        t = time.perf_counter()
        rc = e.lib.gk_lookup_mismatch(e.ctx, q.ctypes.data_as(P(ctypes.c_uint8)), len(q), k, d,
                                      _native.MISMATCH_BOTH_STRANDS if both else 0,
                                      counts.ctypes.data_as(P(ctypes.c_uint64)), None, None, None, None, 0,
                                      ctypes.byref(total))
        dt = time.perf_counter() - t
        e._check(rc)
        return dt

    res = {"box": box, "bases": bases, "contigs": args.contigs, "k": k, "n_kmers": n, "repeats": args.repeats,
           "kmers_per_thread": KERNEL_R, "count_scheme": COUNT_SCHEME, "scan": [], "hits_two_calls": [], "ball": []}
    scan_counts = {}
    for path, m, d, both in itertools.product(paths, ms, ds, (False, True)):
        clear_knobs()
        _native.options["GKM_MISMATCH_PATH"] = path
        q = np.ascontiguousarray(queries[:m])
        counts = np.zeros((m, d + 1), dtype=np.uint64)
        scan(q, d, both, counts)  # warm
        ts = [scan(q, d, both, counts) for _ in range(args.repeats)]
        e.profile_enable(True)
        scan(q, d, both, counts)
        rep = e.profile_report()
        e.profile_enable(False)
        kern = rep.get("mismatch_" + path, {})
        row = {"path": path, "m": m, "d": d, "both_strands": both, "hits": int(counts.sum()),
               "kernel_ms": kern.get("total_ms"), "kernel_launches": kern.get("count"),
               **stats(ts, pairs=float(n) * m)}
        if kern.get("total_ms"):
            row["kernel_pairs_per_s"] = float(n) * m / (kern["total_ms"] * 1e-3)
        res["scan"].append(row)
        print(json.dumps(row), flush=True)
        key = (m, d, both)
        if key in scan_counts:
            assert np.array_equal(scan_counts[key], counts), f"the paths differ at {key}"
        scan_counts[key] = counts.copy()

    # the two-call hits form on the key path (auto), forward
    clear_knobs()
    for m, d in itertools.product(ms, ds):
        q = np.ascontiguousarray(queries[:m])
        e.mismatch_hits(q, d)
        ts = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            out = e.mismatch_hits(q, d)
            ts.append(time.perf_counter() - t)
        row = {"m": m, "d": d, "hits": int(len(out[1])), **stats(ts)}
        res["hits_two_calls"].append(row)
        print(json.dumps(row), flush=True)

    # yardstick: the Hamming ball through gk_lookup (key path, prefix directory), generation not timed
    clear_knobs()
    _native.options["GKM_LOOKUP_PATH"] = "keys"
    mb = args.ball_queries
    qb = np.ascontiguousarray(queries[:mb])
    shells, gen_s = [], 0.0
    for d in range(max(ds) + 1):
        t = time.perf_counter()
        shells.append(ball_shell(qb, d))
        gen_s += time.perf_counter() - t
    for d in ds:
        batch = np.ascontiguousarray(np.concatenate(shells[:d + 1], axis=1).reshape(-1, k))
        first = np.empty(len(batch), dtype=np.uint64)
        count = np.empty(len(batch), dtype=np.uint32)

        def lookup():
            t = time.perf_counter()
            rc = e.lib.gk_lookup(e.ctx, batch.ctypes.data_as(P(ctypes.c_uint8)), len(batch), k,
                                 first.ctypes.data_as(P(ctypes.c_uint64)), count.ctypes.data_as(P(ctypes.c_uint32)))
            dt = time.perf_counter() - t
            e._check(rc)
            return dt

        lookup()  # warm (the first call also builds the directory)
        ts = [lookup() for _ in range(args.repeats)]
        per_query = count.reshape(mb, -1).astype(np.uint64)
        edges = np.cumsum([0] + [s.shape[1] for s in shells[:d + 1]])
        by_d = np.stack([per_query[:, edges[i]:edges[i + 1]].sum(axis=1) for i in range(d + 1)], axis=1)
        equal = bool(np.array_equal(by_d, scan_counts[(mb, d, False)]))
        assert equal, f"the ball route's counts differ from the scan's at d = {d}"
        row = {"m": mb, "d": d, "ball_queries": int(len(batch)), "ball_per_query": int(len(batch) // mb),
               "counts_equal_scan": equal, **stats(ts)}
        res["ball"].append(row)
        print(json.dumps(row), flush=True)
        del batch, first, count
    res["ball_generation_s_not_timed"] = gen_s

    # the condition: at d = 4, m = ball-queries, forward, the scan beats the ball route
    best = {}
    for row in res["scan"]:
        if row["m"] == mb and not row["both_strands"] and row["path"] == "keys":
            best[row["d"]] = row["median_ms"]
    res["scan_vs_ball"] = [{"d": b["d"], "scan_keys_ms": best.get(b["d"]), "ball_ms": b["median_ms"]} for b in res["ball"]]
    print(json.dumps(res["scan_vs_ball"]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    for row in res["scan_vs_ball"]:
        if row["d"] == 4 and row["scan_keys_ms"] is not None:
            assert row["scan_keys_ms"] < row["ball_ms"], f"the scan loses to the ball route at d = 4: {row}"


if __name__ == "__main__":
    main()
