#!/usr/bin/env python3
"""Time the forward score (decode.forwards, sloika/decode.py:108-139; csrc/forward_score.hip) on a batch of chunks, beside the
remap DP (slk_map_to_sequence_batch_f32, the max-plus twin) on the same shapes in the same process.

    python tools/forward_score_time.py [--pairs 1024] [--rows 800] [--states 1025] [--positions 400] [--windows 7] [--launches 5]

The posterior is a random one in the network layout [rows, pairs, states] (uniform draws, squared, normalised: made on the device),
scored where it lies with blank = 0, min_prob = 1e-5 and full = True, as pipeline.Basecaller.score_chunks does; the remap DP gets
the log of the same rows packed read by read, as its entry takes them.  A window is --launches launches between two events; printed
per kernel: the best and the median window (ms per launch), pairs/s and G cells/s (rows x positions).  The windows of the two
kernels alternate after two untimed windows each.  With --check the first pairs are compared with a float64 numpy recursion.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=800)
    ap.add_argument("--states", type=int, default=1025)
    ap.add_argument("--positions", type=int, default=400)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--free", action="store_true", help="full=False")
    ap.add_argument("--no-remap", action="store_true", help="leave the remap DP out")
    ap.add_argument("--check", type=int, default=0, help="compare this many pairs with a float64 numpy recursion")
    a = ap.parse_args()
    import torch
    from sloika_amd import _lib, device as D
    dev = D.device()
    L = _lib.lib()
    B, T, S, P = a.pairs, a.rows, a.states, a.positions
    gen = torch.Generator(device=dev).manual_seed(7)
    post = torch.rand((T, B, S), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    rs = np.random.RandomState(7)
    seq_h = rs.randint(1, S, size=(B, P)).astype(np.int32)
    seq = torch.from_numpy(seq_h.reshape(-1)).to(dev)
    pos_off = (torch.arange(B + 1, dtype=torch.int64) * P).to(dev)
    row_off = torch.arange(B, dtype=torch.int64).to(dev)
    nrow = torch.full((B,), T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    stream = D.stream_ptr()
    kernels = [("forward score (float64)", lambda: _lib.check(L.slk_forward_score_batch_f32(
        post.data_ptr(), S, row_off.data_ptr(), B, nrow.data_ptr(), S, seq.data_ptr(), pos_off.data_ptr(), B, P, 0,
        0 if a.free else 1, 1e-5, score.data_ptr(), stream), "forward score"))]
    if not a.no_remap:
        lt = torch.log(post.transpose(0, 1).contiguous().view(B * T, S) * (1.0 - 1e-5) + 1e-5)
        ev_off = (torch.arange(B + 1, dtype=torch.int64) * T).to(dev)
        ws_off = (torch.arange(B, dtype=torch.int64) * T * P).to(dev)
        ws = torch.empty(B * T * P, dtype=torch.int32, device=dev)
        rscore = torch.empty(B, dtype=torch.float32, device=dev)
        rpath = torch.empty(B * T, dtype=torch.int32, device=dev)
        kernels.append(("remap DP (float32, with traceback)", lambda: _lib.check(L.slk_map_to_sequence_batch_f32(
            lt.data_ptr(), S, ev_off.data_ptr(), seq.data_ptr(), pos_off.data_ptr(), B, P, 5.0, None, None, ws.data_ptr(),
            ws_off.data_ptr(), rscore.data_ptr(), rpath.data_ptr(), stream), "remap")))
    times = [[] for _ in kernels]
    for w in range(-2, a.windows):                       # two untimed windows first: code objects load, the clock settles
        for k, (_, launch) in enumerate(kernels):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            if w >= 0:
                times[k].append(e0.elapsed_time(e1) / a.launches)
    print("pairs %d  rows %d  states %d  positions %d  full %s; %d windows of %d launches, kernels alternating:"
          % (B, T, S, P, not a.free, a.windows, a.launches))
    for (label, _), t in zip(kernels, times):
        best, med = min(t), float(np.median(t))
        print("  %-36s best %8.3f ms  median %8.3f ms  %9.0f pairs/s  %7.2f G cells/s  (%.2f us per row)"
              % (label, best, med, B / best * 1e3, B * T * P / best / 1e6, best * 1e3 / T), flush=True)
        print("      windows (ms):", " ".join("%.3f" % v for v in t), flush=True)
    got = score.cpu().numpy()
    print("  scores: finite %d of %d, mean %.6f" % (int(np.isfinite(got).sum()), B, float(got[np.isfinite(got)].mean())))
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import forward_ref
        worst = 0.0
        for b in range(min(a.check, B)):
            p = post[:, b].cpu().numpy()
            p = (np.float32(1e-5) + np.float32(1.0 - 1e-5) * p).astype(np.float32)
            want = forward_ref.forwards(p, seq_h[b], full=not a.free, blank=0)
            worst = max(worst, abs(got[b] - want) / max(1.0, abs(want)))
        print("  largest relative difference from the float64 numpy recursion over %d pairs: %.3e" % (min(a.check, B), worst))


if __name__ == "__main__":
    main()
