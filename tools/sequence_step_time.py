#!/usr/bin/env python3
"""Time the sequence-loss step (train.SequenceTrainingStep.forward_backward, design/sequence_loss.md) beside the cross-entropy step
(train.TrainingStep.forward_backward) on the same network and inputs, in one process.

    python tools/sequence_step_time.py [--model raw_0.98_rgrgr] [--batch 1024] [--samples 4000] [--windows 5] [--calls 3] [--out FILE.json]

Labels: every output row is blank with probability 1/2, so a chunk of 800 rows carries about 400 positions -- the shape
design/forward_backward.md section 7 is quoted on.  The protocol is tools/forward_backward_time.py's: a window is --calls calls between
two clock readings (each call reads its loss back, so it ends in a device synchronise), the windows of the two steps alternate after
two untimed windows each, and the best and the median window are printed per step.  Then one more sequence step runs under the
package's profiler (HIP events on the launch stream) and the shares of the posterior write, the forward-backward entry and
slk_softmax_seq_grad_f32 are printed with the bytes the kernel moved per second.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="raw_0.98_rgrgr")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--min-prob", type=float, default=1e-5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sloika_amd import _lib, models, profiler, train
    _lib.require_gpu()
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.normal(size=(a.samples, a.batch, 1)).astype(np.float32)).cuda()
    nets = [models.build_model(a.model, klen=5, sd=0.5, seed=11) for _ in range(2)]
    first = nets[0].layers[0]
    To = first.out_len(a.samples) if hasattr(first, "out_len") else a.samples
    labels = (rs.randint(1, nets[0].size, size=(To, a.batch)) * (rs.uniform(size=(To, a.batch)) < 0.5)).astype(np.int32)
    weights = np.ones((To, a.batch), dtype=np.float32)
    labels_d, weights_d = torch.from_numpy(labels).cuda(), torch.from_numpy(weights).cuda()
    seq = train.SequenceTrainingStep(nets[0], min_prob=a.min_prob, full=True)
    xent = train.TrainingStep(nets[1], min_prob=a.min_prob, drop=0)
    # the sequence step takes the host label matrix (it cuts the sequences there), the cross-entropy step the device copy
    steps = [("sequence", lambda: seq.forward_backward(x, labels, None)), ("cross-entropy", lambda: xent.forward_backward(x, labels_d, weights_d))]
    times = [[] for _ in steps]
    res = [None, None]
    for w in range(-2, a.windows):                       # two untimed windows first: code objects load, the clock settles
        for k, (_, call) in enumerate(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                res[k] = call()
            if w >= 0:
                times[k].append(1e3 * (time.perf_counter() - t0) / a.calls)
    rec = profiler.start()
    seq.forward_backward(x, labels, None)
    torch.cuda.synchronize()
    profiler.stop()
    regions = rec.summary()
    npos = float((labels != 0).sum()) / a.batch
    print("%s  batch %d x %d samples -> %d rows of %d states, %.0f positions per chunk; %d windows of %d calls, steps alternating  (%s)"
          % (a.model, a.batch, a.samples, To, nets[0].size, npos, a.windows, a.calls, torch.cuda.get_device_name(0)))
    out = {"model": a.model, "batch": a.batch, "samples": a.samples, "rows": To, "positions_per_chunk": npos, "windows": a.windows,
           "calls": a.calls, "device": torch.cuda.get_device_name(0), "ms": {}, "regions_ms": {}}
    for (label, _), t, r in zip(steps, times, res):
        best, med = min(t), float(np.median(t))
        out["ms"][label] = {"best": best, "median": med, "windows": t}
        print("  %-14s best %8.3f ms  median %8.3f ms   loss %.6f  second value %.4f" % (label, best, med, r[0], r[1]), flush=True)
        print("      windows (ms):", " ".join("%.3f" % v for v in t), flush=True)
    print("  sequence / cross-entropy: %.2f (best windows)" % (min(times[0]) / min(times[1])))
    total = sum(d["ms_total"] for d in regions.values())
    for name, what in (("train_seq_post", "posterior write"), ("forward_backward", "forward-backward entry"),
                       ("train_seq_grad", "slk_softmax_seq_grad_f32")):
        d = regions.get(name)
        if d is None:
            continue
        out["regions_ms"][name] = d["ms_total"]
        print("  %-26s %8.3f ms  (%4.1f %% of the profiled regions' %.3f ms; %.2f TB/s on its %.2f GB)"
              % (what, d["ms_total"], 100.0 * d["ms_total"] / total, total, d["bytes"] / d["ms_total"] / 1e9, d["bytes"] / 1e9))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
