#!/usr/bin/env python3
"""Time of minimizer sampling at the ABI boundary: gk_select_minimizers over a resident genome and
gk_minimizers over a read batch, against the same selection in NumPy, and what the sampled index buys.

Genome: gk_reference_random_bases(--bases) cut into --contigs contigs ("random"), and the same with
every tenth stretch of 10 kb overwritten by A ("polyA": tied ords, the direct scan's worst case).
Reads: --reads reads of --length bases sampled from the genome (none across a contig end).  Per (k, w) of --params and per input:
    select      gk_select_minimizers, host clock around the call (it synchronises), median of --repeats
                warm calls; the two kernel passes alone from the context's timers (gk_profile_enable)
    minimizers  gk_minimizers of the read batch the same way (host arrays in, the view left on the device)
    bandwidth   the passes' bytes -- 1 B read per position and pass, 17 B (4 B for select) written per
                selected position -- over the kernels' time, as a fraction of 8 TB/s
    numpy       sliding_window_view(ord, w).argmin on --numpy-bases bases of the random genome, scaled to
                --bases (labelled scaled; first (k, w) only)
Payoff, first (k, w) only: the sampled index's size and sort time against the full index's, and
Kmers.find_minimizers-style lookups (minimizers on the device, the windows gathered on the host, gk_lookup)
against gk_screen on the same reads: lookups issued per read and time per batch.

    python tools/minimizer_bench.py --out profiles/minimizer/minimizer_1e8.json
"""

import argparse
import json
import platform
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "genome-kmers_amd"))
sys.path.insert(0, str(ROOT / "tests"))

from genome_kmers import _native  # noqa: E402


def make_genome(bases, contigs, seed, poly_a):
    sba = _native.reference_random_bases(bases, seed)
    if poly_a:
        for s in range(0, bases - 10_000, 100_000):
            sba[s:s + 10_000] = 65
    cuts = [bases * i // contigs for i in range(1, contigs)]
    sba[cuts] = 36
    return sba, np.array([0] + [c + 1 for c in cuts], dtype=np.uint32)


def make_reads(sba, nreads, length, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, len(sba) - length + 1, nreads)
    reads = np.empty((nreads, length), dtype=np.uint8)
    for a in range(0, nreads, 1 << 16):
        reads[a:a + (1 << 16)] = sba[s[a:a + (1 << 16), None] + np.arange(length)[None, :]]
    cross = np.flatnonzero((reads == 36).any(axis=1))  # a read across a contig end: taken from the genome's start
    reads[cross] = sba[cross[:, None] % 1000 + np.arange(length)[None, :]]
    return reads.reshape(-1), np.arange(nreads + 1, dtype=np.uint64) * np.uint64(length)


def timed(fn, repeats):
    fn()  # warm
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "spread": round((ms[-1] - ms[0]) / med, 3)}


def kernel_ms(e, fn):
    e.profile_enable(True)
    fn()
    rep = e.profile_report()
    e.profile_enable(False)
    return {name: round(v["total_ms"], 3) for name, v in rep.items() if name.startswith("minimizer_")}


def box_info():
    import torch

    prop = torch.cuda.get_device_properties(0)
    return {"gpu": prop.name, "gcn_arch": getattr(prop, "gcnArchName", ""), "hip": torch.version.hip,
            "host": platform.node()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--params", default="15:10,21:11,31:19,31:200")
    ap.add_argument("--numpy-bases", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--no-payoff", action="store_true", help="selection times only (A/B runs of variant builds: GKM_LIB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bases, nreads = int(args.bases), int(args.reads)
    params = [tuple(map(int, p.split(":"))) for p in args.params.split(",")]
    assert _native.device_count() > 0, "minimizer_bench needs a GPU"
    out = {"box": box_info(), "bases": bases, "reads": nreads, "length": args.length, "repeats": args.repeats,
           "timing": "warm, median of the repeats, host clock around synchronising calls; kernels from the context's timers",
           "inputs": {}}
    for name in ("random", "polyA"):
        sba, seg = make_genome(bases, args.contigs, args.seed, name == "polyA")
        reads, offsets = make_reads(sba, nreads, args.length, args.seed + 1)
        e = _native.Engine()
        e.set_sequence(sba, seg)
        rows = []
        for k, w in params:
            row = {"k": k, "w": w}
            n = e.select_minimizers(k, w, 0)
            row["select"] = timed(lambda: e.select_minimizers(k, w, 0), args.repeats)
            row["select"]["selected"] = n
            row["select"]["positions_per_s"] = round(bases / row["select"]["ms"] * 1e3)
            ker = kernel_ms(e, lambda: e.select_minimizers(k, w, 0))
            row["select"]["kernels_ms"] = ker
            kms = sum(ker.values())
            if kms:
                row["select"]["fraction_of_8TBs"] = round((2 * bases + 4 * n) / (kms * 1e-3) / 8e12, 4)

            def run_reads():
                cn = np.zeros(1, dtype=np.uint64)
                import ctypes
                e._check(e.lib.gk_minimizers(e.ctx, _native._ptr(reads, ctypes.c_uint8), _native._ptr(offsets, ctypes.c_uint64),
                                             nreads, k, w, 0, _native._ptr(cn, ctypes.c_uint64), None))
                return int(cn[0])

            m = run_reads()
            row["minimizers"] = timed(run_reads, args.repeats)
            row["minimizers"]["selected"] = m
            row["minimizers"]["positions_per_s"] = round(reads.size / row["minimizers"]["ms"] * 1e3)
            ker = kernel_ms(e, run_reads)
            row["minimizers"]["kernels_ms"] = ker
            kms = sum(ker.values())
            if kms:
                row["minimizers"]["fraction_of_8TBs"] = round((2 * reads.size + 17 * m) / (kms * 1e-3) / 8e12, 4)
            rows.append(row)
            print(name, json.dumps(row), flush=True)
        out["inputs"][name] = rows
        if name == "random" and not args.no_payoff:
            k, w = params[0]
            # the same selection in NumPy on a prefix, scaled
            import minimizerref as ref
            from numpy.lib.stride_tricks import sliding_window_view

            nb = min(int(args.numpy_bases), bases)
            sub = sba[:nb]
            t = time.perf_counter()
            valid, ckey, _, _ = ref.position_keys(sub, np.array([0, nb], dtype=np.uint64), k, False)
            o = ref.mix_np(ckey)
            arg = sliding_window_view(o, w).argmin(axis=1)
            ok = sliding_window_view(valid, w).all(axis=1)
            sel = np.zeros(nb, dtype=bool)
            sel[np.flatnonzero(ok) + arg[ok]] = True
            ms = (time.perf_counter() - t) * 1e3
            out["numpy"] = {"k": k, "w": w, "bases": nb, "ms": round(ms, 1), "scaled_to_bases_ms": round(ms * bases / nb, 1),
                            "label": "scaled linearly from the prefix"}
            # payoff: sampled against full index; minimizer lookups against the screen
            pay = {"k": k, "w": w}
            full = _native.Engine()
            full.set_sequence(sba, seg)
            nfull = full.enumerate(k)
            t = time.perf_counter()
            full.sort(k)
            full.sync()
            pay["full"] = {"kmers": nfull, "sort_ms": round((time.perf_counter() - t) * 1e3, 2)}
            ns = e.select_minimizers(k, w, 0)
            t = time.perf_counter()
            e.sort(k)
            e.sync()
            pay["sampled"] = {"kmers": ns, "sort_ms": round((time.perf_counter() - t) * 1e3, 2),
                              "fraction_of_full": round(ns / nfull, 4)}

            def via_minimizers():
                pos, _, _, _ = e.minimizers((reads, offsets), k, w, 0)
                win = np.empty((pos.size, k), dtype=np.uint8)  # the host gather, in blocks
                p64 = pos.astype(np.int64)
                for a in range(0, pos.size, 1 << 21):
                    win[a:a + (1 << 21)] = reads[p64[a:a + (1 << 21), None] + np.arange(k)[None, :]]
                e.lookup(win)
                return pos.size

            lookups = via_minimizers()
            pay["find_minimizers"] = timed(via_minimizers, args.repeats)
            pay["find_minimizers"]["lookups_per_read"] = round(lookups / nreads, 2)
            pay["find_minimizers"]["note"] = "the selected windows are gathered on the host (NumPy) before gk_lookup"
            pay["screen"] = timed(lambda: full.screen(reads, offsets), args.repeats)
            pay["screen"]["lookups_per_read"] = args.length - k + 1
            out["payoff"] = pay
            print("payoff", json.dumps(pay), flush=True)
            del full
        del e
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
