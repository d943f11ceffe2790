#!/usr/bin/env python3
"""Time the remap DP (transducer.map_to_sequence, sloika/transducer.py:14-73) on synthetic reads: the LDS-resident kernel
(slk_map_to_sequence_batch_f32) and, with --long, the tiled one (slk_map_to_sequence_long_batch_f32) at every tile of --tile.

    python tools/remap_time.py [--reads 64] [--events 1800] [--positions 600] [--rounds 7]
    python tools/remap_time.py --events 2000 --positions 5846 --long --tile 0,1024,6784

Posteriors follow a monotone walk through the reference's states plus Dirichlet noise (the generator of
tests/golden/make_remap_goldens.py).  All kernels run in ONE process, alternating round by round after three untimed rounds;
printed per kernel: the median and the smallest round (ms per launch), the spread of its rounds (largest - smallest), reads/s and
G cells/s (events x positions), and whether scores and paths equal those of the first kernel bit for bit.  The LDS-resident kernel
is left out where it refuses the shape (more than 5846 positions).  --experiment names a shared library of an experiment
(tools/experiments/remap_global_scratch.hip) that exports `exp_map_to_sequence_long_batch_f32` with the arguments of
slk_map_to_sequence_long_batch_f32, to be timed beside the library's kernels; every read's workspace then has room for a scratch
of 8 words per position.  With --check the first read is compared with the CPU oracle.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--events", type=int, default=1800)
    ap.add_argument("--positions", type=int, default=600)
    ap.add_argument("--slip", type=float, default=5.0)
    ap.add_argument("--rounds", "--reps", type=int, default=7, dest="rounds")
    ap.add_argument("--long", action="store_true", help="also time the tiled kernel")
    ap.add_argument("--tile", default="0", help="tile lengths for --long, comma separated; 0 is the default tile")
    ap.add_argument("--experiment", default=None, help="a library that exports exp_map_to_sequence_long_batch_f32")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import torch
    import make_remap_goldens as mrg
    from sloika_amd import _lib, device as D
    rs = np.random.RandomState(7)
    base_states = [int(v) for v in rs.randint(1, 1025, size=a.positions)]
    posts = [np.log(np.maximum(mrg.plausible_posterior(np.random.RandomState(100 + r), base_states, a.events), 1e-5)).astype(np.float32)
             for r in range(min(a.reads, 4))]
    dev = D.device()
    nread = a.reads
    L = _lib.lib()
    lt = torch.cat([torch.from_numpy(posts[r % len(posts)]) for r in range(nread)]).to(dev)
    ev_off = torch.arange(nread + 1, dtype=torch.int64) * a.events
    pos_off = torch.arange(nread + 1, dtype=torch.int64) * a.positions
    words = L.slk_map_to_sequence_long_workspace_bytes(a.events, a.positions, 0) // 4        # (the traceback alone is shorter)
    if a.experiment:
        words = max(words, a.events * a.positions + 8 * a.positions + 64)
    ws_off = torch.arange(nread, dtype=torch.int64) * words
    seq = torch.tensor(base_states * nread, dtype=torch.int32)
    ev_off, pos_off, ws_off, seq = (t.to(dev) for t in (ev_off, pos_off, ws_off, seq))
    ws = torch.empty(nread * words, dtype=torch.int32, device=dev)
    stream = D.stream_ptr()

    kernels = []                                         # (label, launch, score, path)

    def add(label, call):
        score = torch.empty(nread, dtype=torch.float32, device=dev)
        path = torch.empty(nread * a.events, dtype=torch.int32, device=dev)
        kernels.append((label, lambda: _lib.check(call(score, path), label), score, path))

    if a.positions <= 5846:
        add("LDS-resident", lambda score, path: L.slk_map_to_sequence_batch_f32(
            lt.data_ptr(), 1025, ev_off.data_ptr(), seq.data_ptr(), pos_off.data_ptr(), nread, a.positions, a.slip, None, None,
            ws.data_ptr(), ws_off.data_ptr(), score.data_ptr(), path.data_ptr(), stream))
    if a.long:
        for tile in (int(t) for t in a.tile.split(",")):
            add("tiled, tile %s" % (tile or "default"), lambda score, path, tile=tile: L.slk_map_to_sequence_long_batch_f32(
                lt.data_ptr(), 1025, ev_off.data_ptr(), seq.data_ptr(), pos_off.data_ptr(), nread, a.positions, a.slip, None, None,
                ws.data_ptr(), ws_off.data_ptr(), tile, score.data_ptr(), path.data_ptr(), stream))
    if a.experiment:
        X = ctypes.CDLL(os.path.abspath(a.experiment))
        X.exp_map_to_sequence_long_batch_f32.argtypes = _lib.PROTOTYPES["slk_map_to_sequence_long_batch_f32"][1]
        add("experiment", lambda score, path: X.exp_map_to_sequence_long_batch_f32(
            lt.data_ptr(), 1025, ev_off.data_ptr(), seq.data_ptr(), pos_off.data_ptr(), nread, a.positions, a.slip, None, None,
            ws.data_ptr(), ws_off.data_ptr(), 0, score.data_ptr(), path.data_ptr(), stream))
    if not kernels:
        raise SystemExit("%d positions: the LDS-resident kernel takes 5846; add --long" % a.positions)

    times = [[] for _ in kernels]
    for rnd in range(-3, a.rounds):                      # three untimed rounds first: code objects load, the clock settles
        for k, (_, launch, _, _) in enumerate(kernels):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            if rnd >= 0:
                times[k].append(e0.elapsed_time(e1))
    cells = nread * a.events * a.positions
    print("reads %d  events %d  positions %d  slip %g, %d rounds, kernels alternating:" % (nread, a.events, a.positions, a.slip, a.rounds))
    for (label, _, score, path), t in zip(kernels, times):
        med, best = float(np.median(t)), min(t)
        same = torch.equal(score.view(torch.int32), kernels[0][2].view(torch.int32)) and torch.equal(path, kernels[0][3])
        print("  %-36s median %9.3f ms  best %9.3f ms  spread %7.3f ms  %7.0f reads/s  %6.2f G cells/s  (%.1f us per event)  "
              "same bits as the first: %s" % (label, med, best, max(t) - min(t), nread / med * 1e3, cells / med / 1e6,
                                              med * 1e3 / a.events, same), flush=True)
        print("      rounds (ms):", " ".join("%.3f" % v for v in t), flush=True)
    if a.check:
        from oracle import oracle
        oracle.build()
        sc, pa = oracle.map_to_sequence(posts[0], base_states, slip=a.slip, log=True)
        for label, _, score, path in kernels:
            got = path[: a.events].cpu().numpy()
            print("  %s vs oracle: score %s path %s" % (label, np.float32(sc) == score[0].item(), np.array_equal(got, pa)))


if __name__ == "__main__":
    main()
