"""genome_kmers.distributed.lookup_counts: two processes, each with its own engine on the GPU and its
key-range shard of one genome (KeyRangeKmerSort over gloo), look one query batch up and all-reduce
the counts.  The sum equals each k-mer's multiplicity in the whole genome, computed on the host by
bisection over the sorted k-mer strings."""

import os
import queue
import socket
from bisect import bisect_left, bisect_right

import numpy as np
import pytest

from genome_kmers import _native
from genome_kmers import distributed as D

pytestmark = pytest.mark.gpu
K = 31


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, sba, seg, queries, q):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        job = D.KeyRangeKmerSort(sba, seg, K, rank, world, device=0, torch_device=torch.device("cpu"))
        job.run()
        _, local = job.engine.lookup(queries)
        total = D.lookup_counts(job.engine, queries)
        q.put((rank, job.local_kmers, local.tolist(), total.tolist()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_sum_to_the_global_multiplicity():
    import torch.multiprocessing as mp

    assert _native.device_count() > 0, "gpu tests need a visible MI355X"
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    sba = acgt[rng.integers(0, 4, 60_000)].copy()
    sba[40_000:40_600] = sba[1000:1600]    # repeats: equal k-mers from both position shares
    sba[50_000:50_200] = sba[1000:1200]
    sba[25_000] = 36                       # two contigs
    seg = np.array([0, 25_001], dtype=np.uint32)
    raw = bytes(sba)
    t = sorted(x for x in (raw[s:s + K] for s in range(len(raw) - K + 1)) if b"$" not in x)
    present = [t[i] for i in rng.integers(0, len(t), 1500)] + [raw[1000 + j:1000 + j + K] for j in range(0, 500, 25)]
    absent = [bytes(r) for r in acgt[rng.integers(0, 4, (1500, K))]]
    queries = _native.pack_queries(present + absent)
    want = [bisect_right(t, x) - bisect_left(t, x) for x in present + absent]
    assert max(want) == 3 and want.count(0) >= 1400

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, sba, seg, queries, q)) for r in range(2)]
    res = []
    try:
        for p in procs:
            p.start()
        for _ in procs:
            try:
                res.append(q.get(timeout=120))
            except queue.Empty:
                break  # a worker died or hangs: its exit code below says which
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
                p.join()
    assert [p.exitcode for p in procs] == [0, 0]
    res.sort()
    assert len(res) == 2
    assert sum(r[1] for r in res) == len(t) and all(r[1] > 0 for r in res)
    assert res[0][3] == want and res[1][3] == want            # the all-reduced counts, on every rank
    local = np.array([r[2] for r in res])
    assert (local.sum(axis=0) == np.array(want)).all()
    assert ((local > 0).sum(axis=0) <= 1).all()               # a k-mer is owned by exactly one rank
    assert (local[0] > 0).any() and (local[1] > 0).any()
