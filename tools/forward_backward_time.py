#!/usr/bin/env python3
"""Time forward-backward (csrc/forward_backward.hip, design/forward_backward.md) on a batch of chunks, beside the forward score
(slk_forward_score_batch_f32) on the same shapes in the same process.

    python tools/forward_backward_time.py [--pairs 1024] [--rows 800] [--states 1025] [--positions 400] [--windows 7] [--launches 5]

The posterior is the one tools/forward_score_time.py makes: random, in the network layout [rows, pairs, states], read where it lies
with blank = 0, min_prob = 1e-5 and full = True, as pipeline.Basecaller.occupancy_chunks does.  A window is --launches launches
between two events; printed per kernel: the best and the median window (ms per launch) and the ratio of the best windows.  The windows
of the two kernels alternate after two untimed windows each.  A forward-backward launch is the whole entry: the copy of the lengths to
the host, the zero-fill of occ and the kernel.  With --check the first pairs are compared with the float64 numpy oracle of the tests.
"""
import argparse
import ctypes
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
    ap.add_argument("--check", type=int, default=0, help="compare this many pairs with the float64 numpy oracle")
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
    pos_h = np.arange(B + 1, dtype=np.int64) * P
    nrow_h = np.full(B, T, dtype=np.int32)
    pos_off = torch.from_numpy(pos_h).to(dev)
    row_off = torch.arange(B, dtype=torch.int64).to(dev)
    nrow = torch.from_numpy(nrow_h).to(dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    score_fb = torch.empty(B, dtype=torch.float64, device=dev)
    occ = torch.empty((T, B, S), dtype=torch.float32, device=dev)
    emit_row = torch.empty(B * P, dtype=torch.int32, device=dev)
    emit_prob = torch.empty(B * P, dtype=torch.float64, device=dev)
    need = int(L.slk_forward_backward_workspace_bytes(B, nrow_h.ctypes.data_as(ctypes.c_void_p), pos_h.ctypes.data_as(ctypes.c_void_p)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = D.stream_ptr()
    full = 0 if a.free else 1
    common = (post.data_ptr(), S, row_off.data_ptr(), B, nrow.data_ptr(), S, seq.data_ptr(), pos_off.data_ptr(), B, P, 0, full, 1e-5)
    kernels = [("forward score", lambda: _lib.check(L.slk_forward_score_batch_f32(*common, score.data_ptr(), stream), "forward score")),
               ("forward-backward", lambda: _lib.check(L.slk_forward_backward_batch_f32(
                   *common, score_fb.data_ptr(), occ.data_ptr(), S, emit_row.data_ptr(), emit_prob.data_ptr(), ws.data_ptr(), need, stream),
                   "forward-backward"))]
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
    print("pairs %d  rows %d  states %d  positions %d  full %s; workspace %.2f GB; %d windows of %d launches, kernels alternating:"
          % (B, T, S, P, not a.free, need / 1e9, a.windows, a.launches))
    for (label, _), t in zip(kernels, times):
        best, med = min(t), float(np.median(t))
        print("  %-18s best %8.3f ms  median %8.3f ms  %9.0f pairs/s  (%.2f us per row)" % (label, best, med, B / best * 1e3, best * 1e3 / T),
              flush=True)
        print("      windows (ms):", " ".join("%.3f" % v for v in t), flush=True)
    print("  forward-backward / forward score: %.2f (best windows)" % (min(times[1]) / min(times[0])))
    got, got_fb = score.cpu().numpy(), score_fb.cpu().numpy()
    print("  scores: finite %d of %d, the same bits from both entries: %s" % (int(np.isfinite(got).sum()), B, got.tobytes() == got_fb.tobytes()))
    sums = occ[:, :min(B, 8)].sum(dim=2, dtype=torch.float64)
    print("  occ row sums of the first pairs: %.9f .. %.9f" % (float(sums.min()), float(sums.max())))
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import forward_backward_ref
        worst = 0.0
        for b in range(min(a.check, B)):
            p = post[:, b].cpu().numpy()
            p = (np.float32(1e-5) + np.float32(1.0 - 1e-5) * p).astype(np.float32)
            want = forward_backward_ref.forwards_backwards(p, seq_h[b], full=not a.free, blank=0)[1]
            worst = max(worst, float(np.abs(occ[:, b].cpu().numpy() - want).max()))
        print("  largest |occ - float64 numpy oracle| over %d pairs: %.3e" % (min(a.check, B), worst))


if __name__ == "__main__":
    main()
