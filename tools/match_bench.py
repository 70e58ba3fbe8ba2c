#!/usr/bin/env python3
"""Throughput of gk_match at the ABI boundary (host arrays in, host arrays out), per path, against the
same answer through the calls a caller had before it, and against gk_screen on the same batch.

Genome and reads are tools/screen_bench.py's: gk_reference_random_bases(--bases) cut into --contigs
contigs, sorted once at --k; --reads reads of --length bases, half sampled from the genome with 1 %
substitutions and half random A/C/G/T strings.  Variants, alternated inside every repeat so that drift
hits them alike:
    keys          gk_match on the key path (GKM_MATCH_PATH=keys), the three per-position arrays asked for
    keys_totals   the same with the per-position arrays NULL: per-read results only
    bytes         gk_match on the byte path (GKM_MATCH_PATH=bytes), per-position arrays asked for
    host          bisection over the length with gk_lookup: per round every position's probe length, the
                  windows of each length cut on the host (numpy) into an [m, q] matrix, one gk_lookup per
                  length; ceil(log2(k + 1)) rounds; then the per-read reductions with numpy
    screen        gk_screen (key path, per-window counts) on the same batch: one search per window
Each timed call is warm (one untimed call per variant first) and timed with the host clock (the calls
synchronise the stream before they return).  Reported per variant: ms of the median call, positions/s,
min / max and the run-to-run spread (max - min) / median.  A second pass with gk_profile_enable gives
the device time of the kernels alone (match_keys, match_bytes, lookup_*, screen_keys; copies excluded).
Before timing, the routes' answers are compared: keys == bytes == host on all six outputs, keys_totals
on the per-read ones, and where a match has the full length its count equals the screen's window count.

    python tools/match_bench.py --out profiles/match/match_1e8.json
"""

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "genome-kmers_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from genome_kmers import _native  # noqa: E402
from screen_bench import box_info, make_genome, make_reads  # noqa: E402

VARIANTS = ("keys", "keys_totals", "bytes", "host", "screen")
PATH_OF = {"keys": "keys", "keys_totals": "keys", "bytes": "bytes"}


def set_option(name, value):
    if name in _native.options:
        del _native.options[name]
    if value:
        _native.options[name] = value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, nreads, k, length = int(args.bases), int(args.reads), args.k, args.length
    names = args.variants.split(",")
    assert _native.device_count() > 0, "match_bench needs a GPU"
    box = box_info()

    sba, seg = make_genome(bases, args.contigs, args.seed)
    reads, offsets = make_reads(sba, nreads, length, args.seed + 1)
    total = int(reads.size)
    e = _native.Engine()
    e.set_sequence(sba, seg)
    n = e.enumerate(k)
    t0 = time.perf_counter()
    e.sort(k)
    e.sync()
    sort_s = time.perf_counter() - t0
    del sba

    u8, u32, u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))

    def blank(per_position):
        out = {"longest": np.zeros(nreads, dtype=np.uint32), "longest_pos": np.zeros(nreads, dtype=np.uint32),
               "sum_len": np.zeros(nreads, dtype=np.uint64)}
        if per_position:
            out.update(lengths=np.zeros(total, dtype=np.uint32), first=np.zeros(total, dtype=np.uint64),
                       count=np.zeros(total, dtype=np.uint32))
        return out

    outs = {v: blank(v != "keys_totals") for v in names if v != "screen"}
    screen_out = (np.zeros(nreads, dtype=np.uint32), np.zeros(nreads, dtype=np.uint64), np.zeros(total, dtype=np.uint32))
    host_parts = {}

    def call_match(v):
        set_option("GKM_MATCH_PATH", PATH_OF[v])
        o = outs[v]
        per = "lengths" in o
        t = time.perf_counter()
        rc = e.lib.gk_match(e.ctx, reads.ctypes.data_as(u8), offsets.ctypes.data_as(u64), nreads, 0, 0,
                            o["longest"].ctypes.data_as(u32), o["longest_pos"].ctypes.data_as(u32),
                            o["sum_len"].ctypes.data_as(u64), o["lengths"].ctypes.data_as(u32) if per else None,
                            o["first"].ctypes.data_as(u64) if per else None,
                            o["count"].ctypes.data_as(u32) if per else None)
        dt = time.perf_counter() - t
        e._check(rc)
        return dt

    def call_screen(v):
        set_option("GKM_SCREEN_PATH", "keys")
        t = time.perf_counter()
        rc = e.lib.gk_screen(e.ctx, reads.ctypes.data_as(u8), offsets.ctypes.data_as(u64), nreads, 0,
                             screen_out[0].ctypes.data_as(u32), screen_out[1].ctypes.data_as(u64),
                             screen_out[2].ctypes.data_as(u32))
        dt = time.perf_counter() - t
        e._check(rc)
        return dt

    rounds = int(np.ceil(np.log2(k + 1)))

    def call_host(v):
        """Bisection over the length, in slabs of reads so that the window matrices stay bounded."""
        o = outs[v]
        slab = max(1, (1 << 22) // length)
        t_cut = t_lookup = t_rest = 0.0
        room_one = np.minimum(length - np.arange(length), k).astype(np.int32)  # m per offset in a read
        t = time.perf_counter()
        for r0 in range(0, nreads, slab):
            r1 = min(nreads, r0 + slab)
            ta = time.perf_counter()
            npos = (r1 - r0) * length
            block = reads[r0 * length:r1 * length]
            padded = np.concatenate([block, np.zeros(k, dtype=np.uint8)])
            lo = np.zeros(npos, dtype=np.int32)
            hi = np.tile(room_one, r1 - r0)
            first = np.zeros(npos, dtype=np.uint64)
            count = np.zeros(npos, dtype=np.uint32)
            t_rest += time.perf_counter() - ta
            for _ in range(rounds):
                ta = time.perf_counter()
                mid = (lo + hi + 1) >> 1
                open_ = lo < hi
                t_rest += time.perf_counter() - ta
                for q in np.unique(mid[open_]).tolist():
                    ta = time.perf_counter()
                    at = np.flatnonzero(open_ & (mid == q))
                    win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(padded, q)[at])
                    tb = time.perf_counter()
                    f = np.empty(len(at), dtype=np.uint64)
                    c = np.empty(len(at), dtype=np.uint32)
                    e._check(e.lib.gk_lookup(e.ctx, win.ctypes.data_as(u8), len(at), q, f.ctypes.data_as(u64),
                                             c.ctypes.data_as(u32)))
                    tc = time.perf_counter()
                    hit = c > 0
                    lo[at[hit]] = q
                    first[at[hit]] = f[hit]
                    count[at[hit]] = c[hit]
                    hi[at[~hit]] = q - 1
                    t_cut += tb - ta
                    t_lookup += tc - tb
                    t_rest += time.perf_counter() - tc
            ta = time.perf_counter()
            sl = slice(r0 * length, r1 * length)
            o["lengths"][sl] = lo
            o["first"][sl] = first
            o["count"][sl] = count
            per_read = lo.reshape(r1 - r0, length)
            o["longest"][r0:r1] = per_read.max(axis=1)
            o["longest_pos"][r0:r1] = per_read.argmax(axis=1)
            o["sum_len"][r0:r1] = per_read.sum(axis=1, dtype=np.uint64)
            t_rest += time.perf_counter() - ta
        dt = time.perf_counter() - t
        host_parts.update(cut_s=t_cut, lookup_s=t_lookup, rest_s=t_rest, rounds=rounds)
        return dt

    def call(v):
        return call_host(v) if v == "host" else call_screen(v) if v == "screen" else call_match(v)

    first_call = {v: call(v) for v in names}  # cold: code objects, scratch, pinned staging, the directory
    # the routes agree before anything is timed
    full = [v for v in names if v in ("keys", "bytes", "host")]
    for v in full[1:]:
        for out in outs[v]:
            assert np.array_equal(outs[v][out], outs[full[0]][out]), f"{v} differs from {full[0]} in {out}"
    if "keys_totals" in names and full:
        for out in ("longest", "longest_pos", "sum_len"):
            assert np.array_equal(outs["keys_totals"][out], outs[full[0]][out]), f"keys_totals differs in {out}"
    if "screen" in names and full:
        at_k = outs[full[0]]["lengths"] == k
        assert np.array_equal(outs[full[0]]["count"][at_k], screen_out[2][at_k]) and not screen_out[2][~at_k].any()

    times = {v: [] for v in names}
    for _ in range(args.repeats):
        for v in names:
            times[v].append(call(v))

    # device time of the kernels alone, in a pass of its own
    kernels = {}
    e.profile_enable(True)
    for v in names:
        call(v)
        rep = e.profile_report()
        kernels[v] = {name: {"count": r["count"], "total_ms": r["total_ms"], "units": r["units"]}
                      for name, r in rep.items() if name.startswith(("match_", "screen_", "lookup_"))}
        e.profile_enable(False)
        e.profile_enable(True)
    e.profile_enable(False)
    set_option("GKM_MATCH_PATH", None)
    set_option("GKM_SCREEN_PATH", None)

    ref = outs[full[0]] if full else None
    res = {"box": box, "note": args.note, "bases": bases, "contigs": args.contigs, "k": k, "n_kmers": n,
           "reads": nreads, "read_length": length, "positions": total, "repeats": args.repeats, "sort_s": sort_s,
           "mean_match_length": float(ref["sum_len"].sum(dtype=np.uint64)) / total if ref else None,
           "positions_at_full_length_fraction": float((ref["lengths"] == k).mean()) if ref else None,
           "host_route_parts_last_call": host_parts, "variants": {}, "kernels_profiled_pass": kernels}
    for v in names:
        ts = sorted(times[v])
        med = ts[len(ts) // 2]
        res["variants"][v] = {"median_ms": med * 1e3, "min_ms": ts[0] * 1e3, "max_ms": ts[-1] * 1e3,
                              "positions_per_s": total / med, "spread": (ts[-1] - ts[0]) / med,
                              "first_call_s": first_call[v], "calls_s": times[v]}
    if "keys" in names and "host" in names:
        a, b = res["variants"]["keys"], res["variants"]["host"]
        res["host_over_keys"] = b["median_ms"] / a["median_ms"]
        res["keys_ahead_by_more_than_the_spreads"] = bool(
            b["median_ms"] - a["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]))
    if "keys" in names and "screen" in names:
        res["keys_over_screen"] = res["variants"]["keys"]["median_ms"] / res["variants"]["screen"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
