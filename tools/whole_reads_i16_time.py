#!/usr/bin/env python3
"""The whole-read mode from int16 ADC samples against the same reads as float64 picoamperes: the bench's whole-read set (bench.synthetic_reads)
turned into int16 plus per-read scaling (varied offsets and ranges, digitisation 8192) with their float64 twins
((adc + offset) * (range / digitisation), what fast5.Fast5.get_read returns), then Basecaller.call_reads_bucketed timed from the float64 host
arrays, from the int16 host arrays with `scaling=`, and on the prepared batches resident in HBM (bench.py's `whole_reads` value).  The
int16 and float64 calls must agree bit for bit.  One JSON line.     python tools/whole_reads_i16_time.py [nreads] [--reps N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from sloika_amd import models, pipeline  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 4096
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
net = models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=11))
rs = np.random.RandomState(0xadc)
trip = np.stack([rs.uniform(-20.0, 40.0, n), rs.uniform(1300.0, 1600.0, n), np.full(n, 8192.0)], axis=1)     # offset, range, digitisation
adc, pa64 = [], []
for r, t in zip(bench.synthetic_reads(n), trip):
    a = np.clip(np.rint(r.astype(np.float64) / (t[1] / t[2]) - t[0]), -32768, 32767).astype(np.int16)
    adc.append(a)
    pa64.append((a.astype(np.float64) + t[0]) * (t[1] / t[2]))
nsamp_raw = sum(len(a) for a in adc)
kw = dict(kmer_len=5, skip=0.0)
lanes = pipeline.Basecaller.read_lanes(net, 8, **kw)


def call(reads, **extra):
    return pipeline.Basecaller.call_reads_bucketed(net, reads, max_batch=256, max_waste=0.08, lanes=lanes, **extra, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


# warm-up as bench.py does (two calls of each kind: the allocator caches device memory per stream)
for _ in range(2):
    call(pa64)
    call(adc, scaling=trip)
best = {"f64": None, "i16": None, "resident": None}
for _ in range(reps):
    d64, r64 = timed(lambda: call(pa64))
    d16, r16 = timed(lambda: call(adc, scaling=trip))
    assert np.array_equal(r64[0].view(np.uint32), r16[0].view(np.uint32)) and list(r64[2]) == list(r16[2])
    assert all(np.array_equal(a, b) for a, b in zip(r64[1], r16[1]))
    batches, nsamp = pipeline.Basecaller.prepare_read_batches(net, pa64, max_batch=256, max_waste=0.08, **kw)
    dres, _ = timed(lambda: pipeline.Basecaller.run_read_batches(net, batches, len(nsamp), lanes=lanes, **kw))
    del batches
    for k, d in (("f64", d64), ("i16", d16), ("resident", dres)):
        best[k] = d if best[k] is None else min(best[k], d)
used = sum(nsamp)
rate = {k: used / v for k, v in best.items()}
print(json.dumps({
    "reads": n, "raw_samples": nsamp_raw, "samples_called": used, "reps": reps, "unit": "samples/s (best of reps)",
    "host_bytes": {"f64": 8 * nsamp_raw, "i16": 2 * nsamp_raw}, "upload_bytes": {"f64": 4 * nsamp_raw, "i16": 2 * nsamp_raw},
    "from_host_f64": rate["f64"], "from_host_i16": rate["i16"], "resident": rate["resident"],
    "from_host_f64_of_resident": rate["f64"] / rate["resident"], "from_host_i16_of_resident": rate["i16"] / rate["resident"],
    "seconds": best, "bit_identical": True}))
