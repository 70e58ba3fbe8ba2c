#!/usr/bin/env python3
"""Throughput of gk_lookup at the ABI boundary (host arrays in, host arrays out), per path.

Genome: gk_reference_random_bases(--bases) cut into --contigs contigs, sorted once at --k.  Queries:
--queries k-mers, half sampled from the genome's own k-mers and half random A/C/G/T strings.
Variants, alternated inside every repeat so that drift hits them alike:
    bytes      the byte path (GKM_LOOKUP_PATH=bytes)
    keys       the key path without the prefix directory (GKM_LOOKUP_PATH=keys, GKM_LOOKUP_DIR=0)
    keys_dir   the key path with the prefix directory
Each timed call is one gk_lookup of the whole batch, warm (one untimed call per variant first), timed
with the host clock around the call (gk_lookup synchronises the stream before it returns).  Reported
per variant: queries/s of the median call, min / max, and the run-to-run spread (max - min) / median.
The directory's one-off cost is reported apart: the first keys_dir call after the sort against the
warm median, and the build kernel's device time from the context's profile.  A second pass with
gk_profile_enable gives the device time of the lookup kernels alone (copies excluded).  The variants'
outputs are compared with one another (they must be identical).

    python tools/lookup_bench.py --out profiles/lookup/lookup_1e8.json
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

VARIANTS = {
    "bytes": {"GKM_LOOKUP_PATH": "bytes"},
    "keys": {"GKM_LOOKUP_PATH": "keys", "GKM_LOOKUP_DIR": "0"},
    "keys_dir": {"GKM_LOOKUP_PATH": "keys"},
}


def set_variant(name):
    for knob in ("GKM_LOOKUP_PATH", "GKM_LOOKUP_DIR"):
        if knob in _native.options:
            del _native.options[knob]
    for knob, value in VARIANTS[name].items():
        _native.options[knob] = value


def make_genome(bases, contigs, seed):
    sba = _native.reference_random_bases(bases, seed)
    cuts = [bases * i // contigs for i in range(1, contigs)]
    sba[cuts] = 36
    seg = np.array([0] + [c + 1 for c in cuts], dtype=np.uint32)
    return sba, seg


def make_queries(sba, k, m, seed):
    rng = np.random.default_rng(seed)
    half = m // 2
    out = np.empty((m, k), dtype=np.uint8)
    filled = 0
    while filled < half:  # windows of the genome that hold no '$'
        s = rng.integers(0, len(sba) - k + 1, min(half - filled + 1024, 1 << 22))
        win = sba[s[:, None] + np.arange(k)[None, :]]
        win = win[(win != 36).all(axis=1)][: half - filled]
        out[filled:filled + len(win)] = win
        filled += len(win)
    out[half:] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m - half, k))]
    return out[rng.permutation(m)]


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
    ap.add_argument("--queries", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--variants", default="bytes,keys,keys_dir")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, m, k = int(args.bases), int(args.queries), args.k
    names = args.variants.split(",")
    assert _native.device_count() > 0, "lookup_bench needs a GPU"
    box = box_info()

    sba, seg = make_genome(bases, args.contigs, args.seed)
    queries = make_queries(sba, k, m, args.seed + 1)
    e = _native.Engine()
    e.set_sequence(sba, seg)
    n = e.enumerate(k)
    t0 = time.perf_counter()
    e.sort(k)
    e.sync()
    sort_s = time.perf_counter() - t0

    qp = queries.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    outs = {v: (np.empty(m, dtype=np.uint64), np.empty(m, dtype=np.uint32)) for v in names}

    def call(v):
        first, count = outs[v]
        t = time.perf_counter()
        rc = e.lib.gk_lookup(e.ctx, qp, m, k, first.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                             count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        dt = time.perf_counter() - t
        e._check(rc)
        return dt

    # first calls (cold: code objects, scratch allocation, and for keys_dir the directory build)
    first_call = {}
    for v in names:
        set_variant(v)
        first_call[v] = call(v)
    ref = outs[names[0]]
    for v in names[1:]:
        assert np.array_equal(outs[v][0], ref[0]) and np.array_equal(outs[v][1], ref[1]), f"{v} differs from {names[0]}"
    times = {v: [] for v in names}
    for _ in range(args.repeats):
        for v in names:
            set_variant(v)
            times[v].append(call(v))

    # device time of the kernels alone, in a pass of its own (the directory rebuilt after a re-sort)
    kernels = {}
    if "keys_dir" in names:
        e.enumerate(k)
        e.sort(k)
    e.profile_enable(True)
    for v in names:
        set_variant(v)
        call(v)
    rep = e.profile_report()
    e.profile_enable(False)
    for name, r in rep.items():
        if name.startswith("lookup_"):
            kernels[name] = {"count": r["count"], "total_ms": r["total_ms"], "units": r["units"]}

    res = {"box": box, "bases": bases, "contigs": args.contigs, "k": k, "n_kmers": n, "queries": m,
           "present_fraction": float((ref[1] > 0).mean()), "repeats": args.repeats, "sort_s": sort_s,
           "variants": {}, "kernels_profiled_pass": kernels}
    for v in names:
        ts = sorted(times[v])
        med = ts[len(ts) // 2]
        res["variants"][v] = {"median_s": med, "min_s": ts[0], "max_s": ts[-1], "queries_per_s": m / med,
                              "spread": (ts[-1] - ts[0]) / med, "first_call_s": first_call[v], "calls_s": times[v]}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
