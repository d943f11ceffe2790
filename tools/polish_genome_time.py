#!/usr/bin/env python3
"""Time polishing on genome coordinates (csrc/polish_genome.hip, design/polish_genome.md Time).  A record, not a threshold.

    python tools/polish_genome_time.py [--reads 64] [--letters 10000] [--rows 20000] [--kmer 5] [--width 512]

Three figures, each the best and the median of --windows timed repeats after two untimed ones, the device idle in between
(torch.cuda.synchronize round every repeat, wall clock: the entries hold host round trips, which belong to their cost):
  1. polish.letter_edits for --reads windows of --letters letters: count, prefix sums, emit, new symbols, k-mer columns;
  2. beside it the host path it replaces, polish.draft_edits (bio.single_letter_edits + bio.edit_states) on ONE such window, once;
  3. polish.sum_gains for the candidates of figure 1, and a whole polish.rescore_genome beside the share of it spent inside
     decode.rescore_edits_banded_device (the scoring kernels, unchanged), the new kernels' share being the rest.

The reads are synthetic: a random genome, --reads windows of it on alternating strands, each read's call the window's own k-mers entered
at evenly spaced rows and aligned to it letter for letter (hand-made columns: neither the decoder nor the mapper is timed), a random
float32 posterior in the network layout, min_prob = 1e-5.
"""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, windows):
    import torch
    out = []
    for w in range(-2, windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if w >= 0:
            out.append((time.perf_counter() - t0) * 1e3)
    return min(out), float(np.median(out)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--letters", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--kmer", type=int, default=5)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-letters", type=int, default=None, help="letters of the one window the host path is timed on")
    a = ap.parse_args()
    import torch
    from sloika_amd import align, bio, decode, polish, device as D
    dev = D.device()
    B, n, T, k, W = a.reads, a.letters, a.rows, a.kmer, a.width
    S = 4 ** k + 1
    rs = np.random.RandomState(7)
    step = max(n // 8, 1)
    G = n + step * (B - 1)
    text = ''.join('ACGT'[i] for i in rs.randint(0, 4, size=G))
    genome = torch.from_numpy(np.frombuffer(text.encode('ascii'), dtype=np.uint8).copy()).to(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    w0 = np.arange(B, dtype=np.int64) * step
    minus = (np.arange(B) % 2).astype(np.int32)
    win = (up(np.zeros(B, dtype=np.int64)), up(w0), up(w0 + n), up(minus))

    # 1: candidates on the device
    best, med, c = timed(lambda: polish.letter_edits(genome, *win, k, 0, bio.EDIT_KINDS, 2 * k), a.windows)
    print("1. letter_edits: %d windows of %d letters, kmer_len %d: %d candidates, %d new symbols: best %.3f ms, median %.3f ms: %.3f ms per "
          "window" % (B, n, k, c.ncand, int(c.cand_new_off[-1].item()), best, med, best / B), flush=True)

    # 2: the host path on one window
    hn = a.host_letters or n
    t0 = time.perf_counter()
    _, rows, eset = polish.draft_edits(text[:hn], k, bio.EDIT_KINDS, 'ACGT', 0, S)
    host_ms = (time.perf_counter() - t0) * 1e3
    print("2. polish.draft_edits on ONE window of %d letters (host, once): %d candidates in %.1f ms; the device's figure per window is "
          "%.0f times smaller (the host figure is one window's)" % (hn, len(eset), host_ms, host_ms * (float(n) / hn) ** 2 / (best / B)),
          flush=True)
    del rows, eset

    # 3: the sum, and a whole rescore_genome
    gen = torch.Generator(device=dev).manual_seed(7)
    ll = torch.randn(c.ncand, generator=gen, device=dev, dtype=torch.float64)
    score = torch.randn(B, generator=gen, device=dev, dtype=torch.float64)
    sbest, smed, _ = timed(lambda: polish.sum_gains(score, ll, c.cand_pair, c.cand_edit, 0, G), a.windows)
    print("3. sum_gains: %d candidates on %d positions: best %.3f ms, median %.3f ms (the sort by (edit, read) included)"
          % (c.ncand, G, sbest, smed), flush=True)
    post = torch.rand((T, B, S), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    nk = n - k + 1
    paths, mrow = np.zeros((B, nk), dtype=np.int32), np.zeros((B, nk), dtype=np.int32)
    for b in range(B):
        s = text[w0[b]:w0[b] + n]
        s = ''.join({'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}[ch] for ch in reversed(s)) if minus[b] else s
        paths[b] = bio.seq_to_states(s, k)
        mrow[b] = (np.arange(nk, dtype=np.int64) * T) // nk
    rows = np.tile(np.array([n, 0, n, 0, n, n, 0, 0, 0], dtype=np.int32), (B, 1))
    off = np.arange(B + 1, dtype=np.int64) * n
    part = (torch.zeros(B * n, dtype=torch.uint8, device=dev), up(off), up(rows), torch.zeros(B, dtype=torch.int32, device=dev))
    ops = align.Ops(torch.zeros((B, n), dtype=torch.uint8, device=dev), n, up(np.full(B, n, dtype=np.int32)), [part], rows,
                    torch.zeros(B * n, dtype=torch.uint8, device=dev), off, up(off), np.zeros(B, dtype=np.int32))
    index = types.SimpleNamespace(offsets=np.array([0, G], dtype=np.int64), G=G, genome=genome, names=["g"], lengths=np.array([G]))
    info = {'contig': np.zeros(B, dtype=np.int64), 'window_start': w0, 'window_end': w0 + n}
    strand = np.where(minus, '-', '+')
    call = (up(paths), up(np.full(B, nk, dtype=np.int32)), up(mrow))
    steps = up(np.full(B, T, dtype=np.int32))
    inner = []
    entry = decode.rescore_edits_banded_device

    def wrapped(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = entry(*args, **kw)
        torch.cuda.synchronize()
        inner.append((time.perf_counter() - t0) * 1e3)
        return out

    decode.rescore_edits_banded_device = wrapped
    try:
        rbest, rmed, got = timed(lambda: polish.rescore_genome(post, steps, call[0], call[1], call[2], index, rows, strand, info, ops, k,
                                                               width=W, min_prob=1e-5), a.windows)
    finally:
        decode.rescore_edits_banded_device = entry
    share = min(inner[2:])
    used = int((got.status == polish.READ_DONE).sum())
    fin = int(torch.isfinite(got.ll_edit).sum().item())
    print("   rescore_genome: %d reads of %d rows x %d states, windows of %d letters, W = %d, %d reads used, %d of %d candidates finite: "
          "best %.3f ms, median %.3f ms; inside decode.rescore_edits_banded_device %.3f ms (median %.3f); the rest -- windows, candidates, "
          "bands, sum -- %.3f ms = %.1f %% of the scoring share"
          % (B, T, S, n, W, used, fin, int(got.ll_edit.numel()), rbest, rmed, share, float(np.median(inner[2:])), rbest - share,
             100.0 * (rbest - share) / share), flush=True)


if __name__ == "__main__":
    main()
