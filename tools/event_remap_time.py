#!/usr/bin/env python3
"""Time batch.remap_many against a loop of batch.remap on a set of event reads, in one process on one GPU:

    python tools/event_remap_time.py [--reads 64] [--events 2000] [--model tiny_gru] [--repeats 5] [--out profiles/event_remap_time.json]

Both are run once first (code objects, allocator), their scores and paths compared bit for bit, then timed alternately `repeats` times
with a host clock round work that ends in a device synchronise.  Reads are seeded: about `events` events each (0.75 .. 1.25 of it)
against references of about 0.45 bases per event.  Prints one JSON line; --out also writes it to a file.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_reads(nread, nevent, seed=17):
    rs = np.random.RandomState(seed)
    refs, evs = [], []
    for _ in range(nread):
        n = int(rs.randint(int(0.75 * nevent), int(1.25 * nevent) + 1))
        ev = np.zeros(n, dtype=[("start", "f8"), ("length", "f8"), ("mean", "f8"), ("stdv", "f8")])
        ev["mean"] = 90.0 + 12.0 * np.repeat(rs.normal(size=n), 2)[:n] + rs.normal(scale=0.8, size=n)
        ev["stdv"] = np.abs(1.5 + 0.4 * rs.normal(size=n))
        ev["length"] = (rs.geometric(0.1, size=n) + 2) / 4000.0
        ev["start"] = np.concatenate([[0.0], np.cumsum(ev["length"])[:-1]])
        evs.append(ev)
        refs.append(bytes(rs.choice(list(b"ACGT"), size=max(8, int(0.45 * n))).tolist()))
    return refs, evs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--model", default="tiny_gru")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from sloika_amd import _lib, batch, models
    _lib.require_gpu()
    net = models.randomise_zero_layers(models.build_model(args.model, klen=5, sd=0.5, seed=5))
    batch.init_chunk_remap_worker(net, 5, b"ACGT")
    refs, evs = make_reads(args.reads, args.events)
    prior, slip = (25.0, 25.0), 5.0

    def loop():
        out = [batch.remap(r, e, 1e-5, 5, prior, slip) for r, e in zip(refs, evs)]
        torch.cuda.synchronize()
        return out

    def many():
        out = batch.remap_many(refs, evs, 1e-5, 5, prior, slip)
        torch.cuda.synchronize()
        return out

    a, b = loop(), many()                                      # warm-up, and the check that both compute the same
    same = all(np.float32(x[0]).tobytes() == np.float32(y[0]).tobytes() and np.array_equal(x[2], y[2]) for x, y in zip(a, b))
    t_loop, t_many = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        loop()
        t1 = time.perf_counter()
        many()
        t2 = time.perf_counter()
        t_loop.append(t1 - t0)
        t_many.append(t2 - t1)
    nev = int(sum(len(e) for e in evs))
    res = {"what": "batch.remap_many against a loop of batch.remap, host clock round a device synchronise", "model": args.model,
           "reads": args.reads, "events": nev, "positions": int(sum(len(r) - 4 for r in refs)), "repeats": args.repeats,
           "identical": bool(same), "loop_s": t_loop, "many_s": t_many, "loop_median_s": float(np.median(t_loop)),
           "many_median_s": float(np.median(t_many)), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
