#!/usr/bin/env python3
"""Throughput of gk_screen at the ABI boundary (host arrays in, host arrays out), per path, against
the same answer through the host.

Genome: gk_reference_random_bases(--bases) cut into --contigs contigs, sorted once at --k.  Reads:
--reads reads of --length bases, half sampled from the genome with 1 % substitutions and half random
A/C/G/T strings.  Variants, alternated inside every repeat so that drift hits them alike:
    keys        the key path (GKM_SCREEN_PATH=keys)
    bytes       the byte path (GKM_SCREEN_PATH=bytes)
    keys_both   the key path with GK_SCREEN_BOTH_STRANDS
    host        what a caller could do before gk_screen: every window cut on the host into an [m, k]
                ASCII matrix (numpy), gk_lookup, np.add.reduceat per read
Each timed call produces n_present and occurrences per read in host arrays, warm (one untimed call per
variant first), timed with the host clock (gk_screen and gk_lookup synchronise the stream before they
return).  Reported per variant: ms of the median call, windows/s, min / max and the run-to-run spread
(max - min) / median.  A second pass with gk_profile_enable gives the device time of the kernels alone
(copies excluded).  The host-side offset check (gkm_screen_host.h validate_offsets: the only per-call
host work that grows with the batch besides the staging copy) is timed alone through a call that stops
right after it (a batch whose last offset makes the last sequence over-long); so is the alphabet pass
that Kmers.screen adds on the host (_native.pack_sequences of the packed batch).  The variants' outputs
are compared with one another: keys == bytes == host.

    python tools/screen_bench.py --out profiles/screen/screen_1e8.json
"""

import argparse
import ctypes
import json
import platform
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "genome-kmers_amd"))

from genome_kmers import _native  # noqa: E402

VARIANTS = {"keys": ("keys", 0), "bytes": ("bytes", 0), "keys_both": ("keys", _native.SCREEN_BOTH_STRANDS),
            "host": (None, 0)}


def set_path(path):
    if "GKM_SCREEN_PATH" in _native.options:
        del _native.options["GKM_SCREEN_PATH"]
    if path:
        _native.options["GKM_SCREEN_PATH"] = path


def make_genome(bases, contigs, seed):
    sba = _native.reference_random_bases(bases, seed)
    cuts = [bases * i // contigs for i in range(1, contigs)]
    sba[cuts] = 36
    seg = np.array([0] + [c + 1 for c in cuts], dtype=np.uint32)
    return sba, seg


def make_reads(sba, nreads, length, seed):
    """uint8[nreads * length], uint64 offsets: half from the genome (no '$') with 1 % substitutions,
    half random, shuffled."""
    rng = np.random.default_rng(seed)
    half = nreads // 2
    out = np.empty((nreads, length), dtype=np.uint8)
    filled = 0
    while filled < half:
        s = rng.integers(0, len(sba) - length + 1, min(half - filled + 1024, 1 << 18))
        win = sba[s[:, None] + np.arange(length)[None, :]]
        win = win[(win != 36).all(axis=1)][: half - filled]
        out[filled:filled + len(win)] = win
        filled += len(win)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    sub = rng.random((half, length)) < 0.01
    out[:half][sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    out[half:] = acgt[rng.integers(0, 4, (nreads - half, length))]
    out = out[rng.permutation(nreads)]
    offsets = np.arange(nreads + 1, dtype=np.uint64) * np.uint64(length)
    return np.ascontiguousarray(out.reshape(-1)), offsets


def box_info():
    """What the numbers were measured on: GPU name and architecture, ROCm / HIP version, host CPU."""
    import torch

    prop = torch.cuda.get_device_properties(0)
    cpu = ""
    try:
        with open("/proc/cpuinfo") as fh:
            cpu = next((ln.split(":", 1)[1].strip() for ln in fh if ln.startswith("model name")), "")
    except OSError:
        pass
    return {"gpu": prop.name, "gcn_arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
            "hbm_gib": round(prop.total_memory / 2**30, 1), "hip": torch.version.hip, "torch": torch.__version__,
            "cpu": cpu or platform.processor(), "host": platform.node()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--variants", default="keys,bytes,keys_both,host")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, nreads, k, length = int(args.bases), int(args.reads), args.k, args.length
    names = args.variants.split(",")
    assert _native.device_count() > 0, "screen_bench needs a GPU"
    box = box_info()

    sba, seg = make_genome(bases, args.contigs, args.seed)
    reads, offsets = make_reads(sba, nreads, length, args.seed + 1)
    nwin = nreads * (length - k + 1)
    e = _native.Engine()
    e.set_sequence(sba, seg)
    n = e.enumerate(k)
    t0 = time.perf_counter()
    e.sort(k)
    e.sync()
    sort_s = time.perf_counter() - t0
    del sba

    u8, u32, u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
    outs = {v: (np.zeros(nreads, dtype=np.uint32), np.zeros(nreads, dtype=np.uint64)) for v in names}
    host_parts = {}

    def call_screen(v):
        path, flags = VARIANTS[v]
        set_path(path)
        n_present, occ = outs[v]
        t = time.perf_counter()
        rc = e.lib.gk_screen(e.ctx, reads.ctypes.data_as(u8), offsets.ctypes.data_as(u64), nreads, flags,
                             n_present.ctypes.data_as(u32), occ.ctypes.data_as(u64), None)
        dt = time.perf_counter() - t
        e._check(rc)
        return dt

    def call_host(v):
        """Windows cut with numpy, gk_lookup, reduceat: in slabs of reads, so the [m, k] matrix stays bounded."""
        n_present, occ = outs[v]
        slab = max(1, (1 << 24) // (length - k + 1))
        per = length - k + 1
        t_cut = t_lookup = t_reduce = 0.0
        t = time.perf_counter()
        for r0 in range(0, nreads, slab):
            r1 = min(nreads, r0 + slab)
            ta = time.perf_counter()
            block = reads[r0 * length:r1 * length].reshape(r1 - r0, length)
            win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(block, k, axis=1)).reshape(-1, k)
            tb = time.perf_counter()
            m = win.shape[0]
            first = np.empty(m, dtype=np.uint64)
            count = np.empty(m, dtype=np.uint32)
            e._check(e.lib.gk_lookup(e.ctx, win.ctypes.data_as(u8), m, k, first.ctypes.data_as(u64),
                                     count.ctypes.data_as(u32)))
            tc = time.perf_counter()
            idx = np.arange(0, m, per)
            occ[r0:r1] = np.add.reduceat(count.astype(np.uint64), idx)
            n_present[r0:r1] = np.add.reduceat((count > 0).astype(np.uint32), idx)
            td = time.perf_counter()
            t_cut += tb - ta
            t_lookup += tc - tb
            t_reduce += td - tc
        dt = time.perf_counter() - t
        host_parts.update(cut_s=t_cut, lookup_s=t_lookup, reduce_s=t_reduce)
        return dt

    def call(v):
        return call_host(v) if v == "host" else call_screen(v)

    first_call = {v: call(v) for v in names}  # cold: code objects, scratch, pinned staging, the directory
    plain = [v for v in names if VARIANTS[v][1] == 0]
    for v in plain[1:]:
        assert np.array_equal(outs[v][0], outs[plain[0]][0]) and np.array_equal(outs[v][1], outs[plain[0]][1]), \
            f"{v} differs from {plain[0]}"
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
                      for name, r in rep.items() if name.startswith(("screen_", "lookup_"))}
        e.profile_enable(False)
        e.profile_enable(True)
    e.profile_enable(False)

    # the host-side offset check alone: the call stops right after it when the last sequence is over-long
    set_path(None)
    bad = offsets.copy()
    bad[-1] = bad[-2] + np.uint64(1 << 32)
    check_s = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        rc = e.lib.gk_screen(e.ctx, None, bad.ctypes.data_as(u64), nreads, 0, outs[names[0]][0].ctypes.data_as(u32),
                             outs[names[0]][1].ctypes.data_as(u64), None)
        check_s.append(time.perf_counter() - t)
        assert rc == _native.GK_E_ARG
    check_s.sort()

    # Kmers.screen's own per-byte host work before the call: pack_sequences' alphabet pass over an
    # already packed batch (the C ABI, timed above, does not run it)
    pack_s = []
    for _ in range(3):
        t = time.perf_counter()
        _native.pack_sequences((reads, offsets))
        pack_s.append(time.perf_counter() - t)
    pack_s.sort()

    ref = outs[plain[0]]
    res = {"box": box, "note": args.note, "bases": bases, "contigs": args.contigs, "k": k, "n_kmers": n,
           "reads": nreads, "read_length": length, "windows": nwin, "read_bytes": int(reads.size),
           "windows_present_fraction": float(ref[0].sum(dtype=np.uint64)) / nwin, "repeats": args.repeats,
           "sort_s": sort_s, "offset_check_alone_s": {"median": check_s[len(check_s) // 2], "min": check_s[0],
                                                      "max": check_s[-1]},
           "pack_sequences_alone_s": {"median": pack_s[1], "min": pack_s[0], "max": pack_s[-1]},
           "host_route_parts_last_call": host_parts, "variants": {}, "kernels_profiled_pass": kernels}
    for v in names:
        ts = sorted(times[v])
        med = ts[len(ts) // 2]
        res["variants"][v] = {"median_ms": med * 1e3, "min_ms": ts[0] * 1e3, "max_ms": ts[-1] * 1e3,
                              "windows_per_s": nwin / med, "spread": (ts[-1] - ts[0]) / med,
                              "first_call_s": first_call[v], "calls_s": times[v]}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
