#!/usr/bin/env python3
"""Time of gk_join -- the distinct k-mers of genome A looked up in genome B -- per path, against the
route through the host that exists without it.

Genomes: A = gk_reference_random_bases(--bases) cut into --contigs contigs; B = A with a substitution
at each base with probability --rate (another letter of A/C/G/T).  Both sorted once at --k.
Variants, alternated inside every repeat so that drift hits them alike:
    keys    gk_join on the key path (GKM_JOIN_PATH=keys): the streaming merge of the two unique views
    bytes   gk_join forced to the byte path (GKM_JOIN_PATH=bytes): one search per distinct k-mer of A
    host    the route without gk_join: A's unique view and sorted starts read back, each distinct k-mer
            gathered from the host sba as ASCII, and all of them sent through gk_lookup against B
Each timed call is warm (one untimed call per variant first; the unique views stay valid between
calls) and timed with the host clock around calls that synchronise the stream before they return.
Reported per variant: the median call, min / max and the spread (max - min) / median.  A second pass
with gk_profile_enable gives the device time of the join kernels alone; for the key path its
algorithmic bytes -- per distinct k-mer of A the group start (4 B), the key (8 B), the two results
(4 + 4 B) and, where it is shared, A's multiplicity (4 B); per distinct k-mer of B the group start
(4 B), the key (8 B) and the multiplicity (4 B) -- over that time, as a fraction of the 8 TB/s HBM
peak.  The three variants' answers are compared (they must be identical).

    python tools/join_bench.py --out profiles/join/join_1e8.json
"""

import argparse
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

HBM_PEAK = 8e12  # B/s


def substitute(sba, rate, seed):
    """A copy of sba with a different A/C/G/T letter at each base with probability ``rate``."""
    rng = np.random.default_rng(seed)
    out = sba.copy()
    pos = np.flatnonzero((rng.random(len(sba)) < rate) & (sba != 36))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.searchsorted(letters, out[pos])
    out[pos] = letters[(code + rng.integers(1, 4, len(pos))) % 4]
    return out


def sorted_engine(sba, seg, k):
    e = _native.Engine()
    e.set_sequence(sba, seg)
    n = e.enumerate(k)
    e.sort(k)
    e.sync()
    return e, n


def host_route(ea, eb, sba_a, k, chunk=1 << 23):
    """The parent's route: A's distinct k-mers as ASCII on the host, gk_lookup of each in B."""
    group_start, _ = ea.unique_counts()
    starts = ea.copy_starts()[group_start]
    win = np.lib.stride_tricks.sliding_window_view(sba_a, k)
    first = np.empty(len(starts), dtype=np.uint64)
    count = np.empty(len(starts), dtype=np.uint32)
    for at in range(0, len(starts), chunk):
        f, c = eb.lookup(win[starts[at:at + chunk]])
        first[at:at + chunk], count[at:at + chunk] = f, c
    return first, count


def summary(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median_s": med, "min_s": s[0], "max_s": s[-1], "spread": (s[-1] - s[0]) / med, "calls_s": ts}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=7, help="0 leaves the host route out")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, k = int(args.bases), args.k
    assert _native.device_count() > 0, "join_bench needs a GPU"
    box = box_info()

    sba_a, seg = make_genome(bases, args.contigs, args.seed)
    sba_b = substitute(sba_a, args.rate, args.seed + 1)
    ea, n_a = sorted_engine(sba_a, seg, k)
    eb, n_b = sorted_engine(sba_b, seg, k)

    def join(path):
        _native.options["GKM_JOIN_PATH"] = path
        t = time.perf_counter()
        st = ea.join(eb)
        return time.perf_counter() - t, st

    first_call, stats, results = {}, {}, {}
    for path in ("keys", "bytes"):  # (the first call also computes both unique views)
        first_call[path], stats[path] = join(path)
        results[path] = ea.join_result()
    assert stats["keys"] == stats["bytes"], (stats["keys"], stats["bytes"])
    assert all(np.array_equal(x, y) for x, y in zip(results["keys"], results["bytes"])), "the paths differ"
    times = {"keys": [], "bytes": []}
    for _ in range(args.repeats):
        for path in times:
            times[path].append(join(path)[0])

    # the kernels alone, in a pass of its own
    ea.profile_enable(True)
    for path in ("keys", "bytes"):
        for _ in range(args.repeats):
            join(path)
    rep = ea.profile_report()
    ea.profile_enable(False)
    del _native.options["GKM_JOIN_PATH"]
    kernels = {name: {"count": r["count"], "total_ms": r["total_ms"], "ms_per_call": r["total_ms"] / r["count"],
                      "units": r["units"]} for name, r in rep.items() if name.startswith("join_")}
    st = stats["keys"]
    key_bytes = 20 * st["n_distinct_a"] + 4 * st["n_shared"] + 16 * st["n_distinct_b"]
    keys_ms = kernels["join_keys"]["ms_per_call"]
    traffic = {"algorithmic_bytes": key_bytes, "bytes_per_distinct_kmer_of_a": key_bytes / st["n_distinct_a"],
               "join_keys_ms": keys_ms, "achieved_bytes_per_s": key_bytes / (keys_ms * 1e-3),
               "fraction_of_8_tb_s": key_bytes / (keys_ms * 1e-3) / HBM_PEAK}

    res = {"box": box, "bases": bases, "contigs": args.contigs, "k": k, "substitution_rate": args.rate,
           "n_kmers_a": n_a, "n_kmers_b": n_b, "stats": st, "repeats": args.repeats,
           "first_call_s": first_call, "variants": {p: summary(ts) for p, ts in times.items()},
           "kernels_profiled_pass": kernels, "keys_kernel_traffic": traffic}

    if args.host_repeats > 0:
        got = host_route(ea, eb, sba_a, k)  # warm, and checked
        assert all(np.array_equal(x, y) for x, y in zip(got, results["keys"])), "the host route differs"
        ts = []
        for _ in range(args.host_repeats):
            t = time.perf_counter()
            host_route(ea, eb, sba_a, k)
            ts.append(time.perf_counter() - t)
        res["variants"]["host"] = summary(ts)
        # the search kernels of that route alone
        eb.profile_enable(True)
        host_route(ea, eb, sba_a, k)
        rep = eb.profile_report()
        eb.profile_enable(False)
        res["host_route_lookup_kernels"] = {n: {"count": r["count"], "total_ms": r["total_ms"], "units": r["units"]}
                                            for n, r in rep.items() if n.startswith("lookup_")}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
