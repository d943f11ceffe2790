#!/usr/bin/env python3
"""Time the lattice marginals (csrc/lattice_marginals.hip, slk_viterbi_marginals_f32) beside the stand-alone decoder
(slk_viterbi_kmer_f32) on the same posterior, in the same process.

    python tools/lattice_marginals_time.py [--chunks 1024] [--rows 800] [--klen 5] [--windows 7] [--launches 3] [--gamma]

The posterior is a random one in the network layout [rows, chunks, 4^klen + 1] (uniform draws, squared, normalised: made on the
device), decoded with min_prob = 1e-5 and skip_pen = 0 as pipeline.Basecaller does.  A window is --launches launches between two
events; printed per kernel: the best and the median window (ms per launch) and chunks/s.  The windows of the two kernels alternate
after two untimed windows each.  The marginals' workspace is 9 * 4^klen + 20 bytes per row and chunk (7.6 GB at the defaults).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=800)
    ap.add_argument("--klen", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--gamma", action="store_true", help="also write the [rows, chunks, 4^klen] float32 marginals")
    a = ap.parse_args()
    import torch
    from sloika_amd import _lib, device as D
    dev = D.device()
    L = _lib.lib()
    B, T, N = a.chunks, a.rows, 4 ** a.klen
    gen = torch.Generator(device=dev).manual_seed(7)
    post = torch.rand((T, B, N + 1), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    stream = D.stream_ptr()
    score = torch.empty(B, dtype=torch.float32, device=dev)
    path = torch.empty((B, T), dtype=torch.int32, device=dev)
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    rows = torch.empty((B, T), dtype=torch.int32, device=dev)
    conf = torch.empty((B, T), dtype=torch.float64, device=dev)
    logz = torch.empty(B, dtype=torch.float64, device=dev)
    gamma = torch.empty((T, B, N), dtype=torch.float32, device=dev) if a.gamma else None
    need_v = int(L.slk_viterbi_kmer_workspace_bytes(T, B, 4, a.klen))
    need_m = int(L.slk_viterbi_marginals_workspace_bytes(T, B, 4, a.klen))
    if not need_v or not need_m:
        sys.exit("no kernel for klen %d" % a.klen)
    ws = torch.empty(max(need_v, need_m), dtype=torch.uint8, device=dev)
    kernels = [
        ("decoder (slk_viterbi_kmer_f32)", lambda: _lib.check(L.slk_viterbi_kmer_f32(
            post.data_ptr(), T, B, 4, a.klen, 0.0, _lib.POST_RAW, 1e-5, ws.data_ptr(), need_v, score.data_ptr(), path.data_ptr(),
            lens.data_ptr(), stream), "viterbi")),
        ("marginals (slk_viterbi_marginals_f32)", lambda: _lib.check(L.slk_viterbi_marginals_f32(
            post.data_ptr(), T, B, 4, a.klen, 0.0, _lib.POST_RAW, 1e-5, None, ws.data_ptr(), need_m, score.data_ptr(), path.data_ptr(),
            lens.data_ptr(), rows.data_ptr(), conf.data_ptr(), logz.data_ptr(), D.ptr(gamma), stream), "marginals")),
    ]
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
    print("chunks %d  rows %d  k-mers %d  gamma %s; %d windows of %d launches, kernels alternating:"
          % (B, T, N, bool(a.gamma), a.windows, a.launches))
    for (label, _), t in zip(kernels, times):
        best, med = min(t), float(np.median(t))
        print("  %-40s best %9.3f ms  median %9.3f ms  %9.0f chunks/s" % (label, best, med, B / (best * 1e-3)))
    print("  log Z of chunk 0: %.6f; mean confidence of its %d positions: %.4f"
          % (float(logz[0]), int(lens[0]), float(conf[0, :int(lens[0])].mean())))


if __name__ == "__main__":
    main()
