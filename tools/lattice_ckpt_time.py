#!/usr/bin/env python3
"""Time the lattice marginals with checkpointed forward rows (slk_viterbi_marginals_ckpt_f32) beside the stored-row kernel
(slk_viterbi_marginals_f32) on the same posterior, in the same process (design/lattice_marginals.md 8).

    python tools/lattice_ckpt_time.py [--shape a|b|both] [--every 4 8] [--windows 7] [--launches 3]
    python tools/lattice_ckpt_time.py --reads 300 [--read-lengths 40000 100000] [--lanes 4]

Shapes: (a) 1024 chunks of 800 rows of 1025 float32, the shape of tools/lattice_marginals_time.py's record; (b) 64 chunks of 20000
rows, a bucket of whole reads.  The posterior is that tool's (uniform draws, squared, normalised, made on the device), min_prob =
1e-5, skip_pen = 0, no gamma.  The stored-row kernel is the yardstick: it runs as the consecutive launches transducer.WORKSPACE_LIMIT
forces on it (decode.viterbi_marginals_batch's split; the copies of the posterior's columns those launches need are made outside the
windows).  A window is --launches runs between two events; printed per kernel: the best and the median window (ms per run) and the
workspace bytes.  The kernels' windows alternate after two untimed windows each.

--reads: the end-to-end rate of Basecaller.call_reads_bucketed_qual and fastq_bucketed beside Basecaller.call_reads_bucketed (no
qualities) on the same synthetic long reads, the set on the host, on lanes kept over the calls; best of 3 calls each after one
untimed call.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"a": (1024, 800), "b": (64, 20000)}


def time_shape(a, name):
    import torch
    from sloika_amd import _lib, device as D, transducer
    dev = D.device()
    L = _lib.lib()
    B, T = SHAPES[name]
    klen, N = 5, 4 ** 5
    gen = torch.Generator(device=dev).manual_seed(7)
    post = torch.rand((T, B, N + 1), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    stream = D.stream_ptr()

    def outputs():
        return {"score": torch.empty(B, dtype=torch.float32, device=dev), "path": torch.empty((B, T), dtype=torch.int32, device=dev),
                "len": torch.empty(B, dtype=torch.int32, device=dev), "row": torch.empty((B, T), dtype=torch.int32, device=dev),
                "conf": torch.empty((B, T), dtype=torch.float64, device=dev), "logz": torch.empty(B, dtype=torch.float64, device=dev)}

    def tail(o, lo, hi):
        return (o["score"][lo:hi].data_ptr(), o["path"][lo:hi].data_ptr(), o["len"][lo:hi].data_ptr(), o["row"][lo:hi].data_ptr(),
                o["conf"][lo:hi].data_ptr(), o["logz"][lo:hi].data_ptr(), None, stream)

    # the stored-row kernel, split as decode.viterbi_marginals_batch splits it
    alone = int(L.slk_viterbi_marginals_workspace_bytes(T, 1, 4, klen))
    per = max(1, min(B, transducer.WORKSPACE_LIMIT // alone))
    runs = [(lo, min(lo + per, B)) for lo in range(0, B, per)]
    subs = [post if (hi - lo) == B else post[:, lo:hi].contiguous() for lo, hi in runs]
    need_s = int(L.slk_viterbi_marginals_workspace_bytes(T, runs[0][1] - runs[0][0], 4, klen))
    ws = torch.empty(need_s, dtype=torch.uint8, device=dev)
    want = outputs()

    def stored():
        for (lo, hi), sub in zip(runs, subs):
            _lib.check(L.slk_viterbi_marginals_f32(sub.data_ptr(), T, hi - lo, 4, klen, 0.0, _lib.POST_RAW, 1e-5, None, ws.data_ptr(),
                                                   int(L.slk_viterbi_marginals_workspace_bytes(T, hi - lo, 4, klen)),
                                                   *tail(want, lo, hi)), "marginals")

    kernels = [("stored rows, %d launch%s" % (len(runs), "" if len(runs) == 1 else "es"), stored, need_s, want)]
    for every in a.every:
        need = int(L.slk_viterbi_marginals_ckpt_workspace_bytes(T, B, 4, klen, every))
        if need > ws.numel():
            sys.exit("the checkpointed workspace is the larger one?")
        got = outputs()

        def ckpt(every=every, need=need, got=got):
            _lib.check(L.slk_viterbi_marginals_ckpt_f32(post.data_ptr(), T, B, 4, klen, 0.0, _lib.POST_RAW, 1e-5, None, every,
                                                        ws.data_ptr(), need, *tail(got, 0, B)), "marginals_ckpt")

        kernels.append(("checkpointed, every %d rows" % every, ckpt, need, got))
    times = [[] for _ in kernels]
    for w in range(-2, a.windows):                       # two untimed windows first: code objects load, the clock settles
        for k, (_, launch, _, _) in enumerate(kernels):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            if w >= 0:
                times[k].append(e0.elapsed_time(e1) / a.launches)
    print("shape (%s): chunks %d  rows %d  k-mers %d; %d windows of %d runs, kernels alternating:" % (name, B, T, N, a.windows, a.launches))
    for (label, _, need, out), t in zip(kernels, times):
        equal = all(torch.equal(out[k], want[k]) for k in want)
        print("  %-32s best %10.3f ms  median %10.3f ms  workspace %14d bytes  outputs equal the stored rows': %s"
              % (label, min(t), float(np.median(t)), need, equal))


def time_reads(a):
    import torch
    from sloika_amd import models, pipeline
    net = models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=11)
    rs = np.random.RandomState(5)
    lo, hi = a.read_lengths
    base = pipeline.synthetic_chunks(8, chunk_len=hi + 4000, seed=13)
    reads = [base[i % 8][rs.randint(0, 4000):][:n] for i, n in enumerate(rs.randint(lo, hi + 1, size=a.reads))]
    samples = sum(len(r) for r in reads)
    kw = dict(kmer_len=5, skip=0.0)
    # the lanes are kept over the calls, as a server keeps them: torch's allocator caches device memory per stream
    lanes = pipeline.Basecaller.read_lanes(net, a.lanes, **kw)
    flows = [("call_reads_bucketed (no qualities)", lambda: pipeline.Basecaller.call_reads_bucketed(net, reads, lanes=lanes, **kw)[3]),
             ("call_reads_bucketed_qual", lambda: pipeline.Basecaller.call_reads_bucketed_qual(net, reads, lanes=lanes, **kw)[6]),
             ("fastq_bucketed", lambda: pipeline.Basecaller.fastq_bucketed(net, reads, lanes=lanes, **kw))]
    print("%d synthetic reads of %d .. %d samples, %d samples in all; %d lanes kept over the calls; best of 3 calls after one untimed call:"
          % (a.reads, lo, hi, samples, a.lanes))
    for label, call in flows:
        best = None
        for w in range(-1, 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if w >= 0:
                best = dt if best is None else min(best, dt)
        print("  %-36s %8.3f s  %8.1f M samples/s" % (label, best, samples / best * 1e-6))
    stats = res = flows[1][1]()
    print("  buckets %d  lanes %d  rows per checkpoint %d  memory_limit %d  peak_bucket_bytes %d  padded-step waste %.3f"
          % (stats["batches"], stats["lanes"], stats["rows_per_checkpoint"], stats["memory_limit"], stats["peak_bucket_bytes"],
             stats["padded_step_waste"]))
    del res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b", "both"], default="both")
    ap.add_argument("--every", type=int, nargs="+", default=[4, 8], help="rows per checkpoint to time")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="time the end-to-end flows on this many synthetic reads instead")
    ap.add_argument("--read-lengths", type=int, nargs=2, default=[40000, 100000])
    ap.add_argument("--lanes", type=int, default=4, help="lanes of the end-to-end flows")
    a = ap.parse_args()
    if a.reads:
        time_reads(a)
        return
    for name in ("a", "b") if a.shape == "both" else (a.shape,):
        time_shape(a, name)


if __name__ == "__main__":
    main()
