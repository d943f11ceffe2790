#!/usr/bin/env python3
"""A validation batch (validate.ValidationStep) against the workaround it replaces (TrainingStep.forward_backward) on the same
inputs, one process, the two alternating:

    python tools/validate_time.py [--model raw_0.98_rgrgr] [--batch 1024] [--samples 4000] [--rounds 20] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/validate_time.py --rounds 3 --profile-only

Times are host clocks around work that ends in a device synchronise (both calls read their scalars back).  --profile-only runs
the calls without timing them: the kernel statistics of a rocprofv3 run then hold `rounds` + warm-up calls of each.
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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from sloika_amd import _lib, models, train, validate
    _lib.require_gpu()
    net = models.build_model(args.model, klen=5, sd=0.5, seed=11)
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.normal(size=(args.samples, args.batch, 1)).astype(np.float32)).cuda()
    first = net.layers[0]
    To = first.out_len(args.samples) if hasattr(first, "out_len") else args.samples
    labels = torch.from_numpy(rs.randint(0, net.size, size=(To, args.batch)).astype(np.int32)).cuda()
    weights = torch.ones((To, args.batch), dtype=torch.float32, device="cuda")
    step = train.TrainingStep(net, min_prob=0.0, l2=0.0, drop=0)
    fv = validate.wrap_network(net)
    calls = {"validation": lambda: fv(x, labels), "forward_backward": lambda: step.forward_backward(x, labels, weights)}
    for _ in range(args.warmup):
        res = {k: f() for k, f in calls.items()}
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():                       # alternating: both see the same device state and neighbours
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()                                          # (reads its scalars back: ends in a synchronise)
            times[k].append(1e3 * (time.perf_counter() - t0))
    out = {"model": args.model, "batch": args.batch, "samples": args.samples, "rows": To * args.batch, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           # forward_backward at min_prob = 0, drop = 0, unit weights returns the same mean loss; its accuracy is a float32 mean
           "loss": {"validation": res["validation"][0], "forward_backward": res["forward_backward"][0]},
           "ncorrect": res["validation"][1], "forward_backward_accuracy": res["forward_backward"][1]}
    if not args.profile_only:
        out["ms"] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()}
        out["validation_over_forward_backward"] = out["ms"]["validation"]["median"] / out["ms"]["forward_backward"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
