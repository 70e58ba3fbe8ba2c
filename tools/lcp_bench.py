#!/usr/bin/env python3
"""Time of the LCP view and what is read off it -- gk_lcp, gk_lcp_spectrum, gk_position_track -- against
the routes that exist without them.

Genome: gk_reference_random_bases(--bases) cut into --contigs contigs (``--genome doubled``: its first
half twice, so every k-mer has a twin and lcp piles onto the cap), sorted once at --k.
Variants, alternated inside every repeat so that drift hits them alike:
    spectrum        gk_lcp_spectrum(k) with the view cached: distinct[1..k] and unique[1..k] in one pass
    spectrum_cold   the same right after a sort (untimed), so the call also builds the view
    loop            the route without it: k calls of gk_group_hist(kmer_len, keep-all, max_counts_bin 2),
                    distinct = the histogram's sum, unique = its bin 1
    min_unique      gk_position_track(GK_TRACK_MIN_UNIQUE, k) into a host array (view cached)
    multiplicity    gk_position_track(GK_TRACK_MULTIPLICITY, k) into a host array
    host_mult       the route without it: the unique view and the sorted starts read back, np.repeat of
                    the counts and a NumPy scatter into a zeroed uint32[len(sba)]
    host_min_unique the array read back (gk_copy_lcp) with the starts, the pair maximum and the scatter
                    in NumPy -- what a caller of gk_lcp alone would do (the parent has no route at all)
Each timed call is warm (one untimed call per variant first) and timed with the host clock around calls
that synchronise the stream before they return.  Reported per variant: the median call, min / max and
the spread (max - min) / median.  A second pass with gk_profile_enable gives the device time of the
kernels alone: lcp_keys against its algorithmic 12 B per k-mer (8 read, 4 written) at the 8 TB/s HBM
peak, and track_min_unique against the floor of one random 4-byte store per k-mer at 36 G lines/s
(README.md's figure).  The answers of the routes are compared (they must be identical).

    python tools/lcp_bench.py --out profiles/lcp/lcp_1e8.json
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
RANDOM_LINES = 36e9  # random 64-byte lines / s (README.md)
KEEP_ALL = _native.GkFilter(_native.FILTER_KEEP_ALL, 0, 0, 0, 0)


def summary(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median_s": med, "min_s": s[0], "max_s": s[-1], "spread": (s[-1] - s[0]) / med, "calls_s": ts}


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def log(msg):
    print(f"[lcp_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--genome", choices=("random", "doubled"), default="random")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=7, help="repeats of loop and the host routes; 0 leaves them out")
    ap.add_argument("--spectrum-only", action="store_true", help="the spectrum kernel's device time alone (A/B builds)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, k = int(args.bases), args.k
    assert _native.device_count() > 0, "lcp_bench needs a GPU"

    sba, seg = make_genome(bases, args.contigs, args.seed)
    if args.genome == "doubled":
        half = len(sba) // 2
        sba[half + 1:] = sba[:len(sba) - half - 1]
        sba[half] = 36
        seg = np.concatenate([[0], np.flatnonzero(sba == 36) + 1]).astype(np.uint32)
    L = len(sba)
    e = _native.Engine()
    e.set_sequence(sba, seg)

    def fresh_sort():
        n = e.enumerate(k)
        e.sort(k)
        e.sync()
        return n

    n = fresh_sort()
    log(f"sorted {n} k-mers")

    if args.spectrum_only:
        e.lcp_spectrum(k)
        e.profile_enable(True)
        for _ in range(args.repeats):
            e.lcp_spectrum(k)
        rep = e.profile_report()["lcp_spectrum"]
        d, u = e.lcp_spectrum(k)
        print(json.dumps({"genome": args.genome, "n_kmers": n, "lib": str(_native.LIB_PATH.name),
                          "spectrum_ms": rep["total_ms"] / rep["count"], "distinct_k": int(d[k]), "unique_k": int(u[k])}))
        return
    box = box_info()

    def loop():
        distinct, unique = np.zeros(k + 1, dtype=np.int64), np.zeros(k + 1, dtype=np.int64)
        for q in range(1, k + 1):
            hist, _ = e.group_hist(1, q, KEEP_ALL, 1, None, 2)
            distinct[q], unique[q] = hist.sum(), hist[1]
        return distinct, unique

    def host_mult():
        group_start, counts = e.unique_counts()
        starts = e.copy_starts()
        track = np.zeros(L, dtype=np.uint32)
        track[starts] = np.repeat(counts, counts)
        return track

    def host_min_unique():
        v = e.lcp(k)
        starts = e.copy_starts()
        m = np.maximum(v, np.append(v[1:], np.uint32(0)))
        track = np.zeros(L, dtype=np.uint32)
        track[starts] = np.where(m < k, m + 1, np.uint32(_native.NEVER_UNIQUE))
        return track

    variants = {
        "spectrum": lambda: e.lcp_spectrum(k),
        "min_unique": lambda: e.position_track(_native.TRACK_MIN_UNIQUE, k, L),
        "multiplicity": lambda: e.position_track(_native.TRACK_MULTIPLICITY, k, L),
    }
    slow = {"loop": loop, "host_mult": host_mult, "host_min_unique": host_min_unique} if args.host_repeats > 0 else {}

    # the first calls, checked against each other (large arrays are dropped as soon as they are compared)
    first_call = {}
    first_call["spectrum_cold"], spectrum = timed(variants["spectrum"])  # builds the view
    if slow:
        first_call["loop"], got = timed(loop)
        assert all(np.array_equal(x, y) for x, y in zip(spectrum, got)), "spectrum != loop"
    for name, host in (("min_unique", "host_min_unique"), ("multiplicity", "host_mult")):
        log(f"first calls: {name}")
        first_call[name], track = timed(variants[name])
        if slow:
            first_call[host], got = timed(slow[host])
            assert np.array_equal(track, got), f"{name} != {host}"
            del got
        del track

    times = {name: [] for name in list(variants) + ["spectrum_cold"]}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            times[name].append(timed(fn)[0])
        fresh_sort()  # untimed: drops the view
        times["spectrum_cold"].append(timed(variants["spectrum"])[0])
    slow_times = {name: [] for name in slow}
    for _ in range(args.host_repeats):
        for name, fn in slow.items():
            slow_times[name].append(timed(fn)[0])
            log(f"{name}: {slow_times[name][-1]:.3f} s")

    # the kernels alone, in a pass of its own
    log("profiled pass")
    e.profile_enable(True)
    for _ in range(args.repeats):
        fresh_sort()
        for fn in variants.values():
            fn()
    if slow:
        loop()
    rep = e.profile_report()
    e.profile_enable(False)
    names = ("lcp_keys", "lcp_bytes", "lcp_spectrum", "track_min_unique", "track_multiplicity", "group_heads",
             "group_hist")
    kernels = {name: {"count": r["count"], "total_ms": r["total_ms"], "ms_per_call": r["total_ms"] / r["count"],
                      "units": r["units"]} for name, r in rep.items() if name in names}
    words = e.key_layout()[0]
    lcp_bytes = (8 * words + 4) * n
    lcp_ms = kernels["lcp_keys"]["ms_per_call"]
    scatter_ms = kernels["track_min_unique"]["ms_per_call"]
    model = {
        "lcp_keys": {"algorithmic_bytes": lcp_bytes, "bytes_per_kmer": 8 * words + 4, "ms": lcp_ms,
                     "floor_ms_at_8_tb_s": lcp_bytes / HBM_PEAK * 1e3,
                     "achieved_bytes_per_s": lcp_bytes / (lcp_ms * 1e-3),
                     "fraction_of_8_tb_s": lcp_bytes / (lcp_ms * 1e-3) / HBM_PEAK},
        "track_min_unique": {"ms": scatter_ms, "scatter_floor_ms_at_36_g_lines_s": n / RANDOM_LINES * 1e3,
                             "stores_per_s": n / (scatter_ms * 1e-3)},
    }
    res = {"box": box, "bases": bases, "contigs": args.contigs, "k": k, "genome": args.genome, "n_kmers": n,
           "sba_len": L, "distinct_k": int(spectrum[0][k]), "unique_k": int(spectrum[1][k]),
           "repeats": args.repeats, "host_repeats": args.host_repeats, "first_call_s": first_call,
           "variants": {name: summary(ts) for name, ts in {**times, **slow_times}.items()},
           "kernels_profiled_pass": kernels, "model": model}
    if slow:
        v = res["variants"]
        res["ratios"] = {
            "loop_over_spectrum_warm": v["loop"]["median_s"] / v["spectrum"]["median_s"],
            "loop_over_spectrum_cold": v["loop"]["median_s"] / v["spectrum_cold"]["median_s"],
            "host_mult_over_multiplicity": v["host_mult"]["median_s"] / v["multiplicity"]["median_s"],
            "host_min_unique_over_min_unique": v["host_min_unique"]["median_s"] / v["min_unique"]["median_s"],
        }
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
