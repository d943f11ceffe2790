#!/usr/bin/env python3
"""Time variants of any length on genome coordinates (csrc/polish_variants.hip, design/polish_variants.md Time).  A record, not a
threshold.

    python tools/polish_variants_time.py [--reads 64] [--letters 10000] [--rows 20000] [--kmer 5] [--width 512]

Each figure is the best and the median of its timed repeats (--launches for figures 1 to 3, --windows for 4) after two untimed ones,
the device idle in between (torch.cuda.synchronize round every repeat, wall clock: the entries hold host round trips, which belong to
their cost):
  1. polish.repeat_variants of the whole genome: count, prefix sums, emit;
  2. polish.variant_edits of those proposals for --reads windows of --letters letters: status, count, prefix sums, emit, new symbols,
     k-mer columns;
  3. polish.sum_variant_gains for the candidates of figure 2, torch's two stable sorts included;
  4. a whole polish.rescore_variants(variants='repeats') beside polish.rescore_genome on the same reads, each with the share of it
     spent inside decode.rescore_edits_banded_device (the scoring kernels, unchanged).

The reads are polish_genome_time.py's: a random genome, --reads windows of it on alternating strands, each read's call the window's own
k-mers entered at evenly spaced rows and aligned to it letter for letter (hand-made columns: neither the decoder nor the mapper is
timed), a random float32 posterior in the network layout, min_prob = 1e-5.
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
    ap.add_argument("--windows", type=int, default=5, help="timed repeats of the whole rescoring calls")
    ap.add_argument("--launches", type=int, default=200, help="timed repeats of figures 1 to 3")
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
    index = types.SimpleNamespace(offsets=np.array([0, G], dtype=np.int64), G=G, genome=genome, names=["g"], lengths=np.array([G]))

    best, med, vs = timed(lambda: polish.repeat_variants(index, k), a.launches)
    print("1. repeat_variants: %d letters, kmer_len %d: %d proposals, %d alt letters: best %.3f ms, median %.3f ms"
          % (G, k, vs.V, vs.A, best, med), flush=True)

    best, med, c = timed(lambda: polish.variant_edits(genome, vs.contig_off, *win, vs, k, 0, 2 * k), a.launches)
    print("2. variant_edits: %d windows of %d letters: %d candidates, %d new symbols: best %.3f ms, median %.3f ms: %.3f ms per window"
          % (B, n, c.ncand, int(c.cand_new_off[-1].item()), best, med, best / B), flush=True)

    gen = torch.Generator(device=dev).manual_seed(7)
    ll = torch.randn(c.ncand, generator=gen, device=dev, dtype=torch.float64)
    score = torch.randn(B, generator=gen, device=dev, dtype=torch.float64)
    sbest, smed, _ = timed(lambda: polish.sum_variant_gains(score, ll, c.cand_pair, c.cand_var, win[3], vs.V), a.launches)
    print("3. sum_variant_gains: %d candidates on %d variants: best %.3f ms, median %.3f ms (the sort by (variant, read) included)"
          % (c.ncand, vs.V, sbest, smed), flush=True)

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
    info = {'contig': np.zeros(B, dtype=np.int64), 'window_start': w0, 'window_end': w0 + n}
    strand = np.where(minus, '-', '+')
    call = (up(paths), up(np.full(B, nk, dtype=np.int32)), up(mrow))
    steps = up(np.full(B, T, dtype=np.int32))
    entry = decode.rescore_edits_banded_device
    for name, fn in (("rescore_variants('repeats')", lambda: polish.rescore_variants(post, steps, call[0], call[1], call[2], index, rows,
                                                                                     strand, info, ops, k, 'repeats', width=W, min_prob=1e-5)),
                     ("rescore_genome", lambda: polish.rescore_genome(post, steps, call[0], call[1], call[2], index, rows, strand, info, ops,
                                                                      k, width=W, min_prob=1e-5))):
        inner = []

        def wrapped(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = entry(*args, **kw)
            torch.cuda.synchronize()
            inner.append((time.perf_counter() - t0) * 1e3)
            return out

        decode.rescore_edits_banded_device = wrapped
        try:
            rbest, rmed, got = timed(fn, a.windows)
        finally:
            decode.rescore_edits_banded_device = entry
        share = min(inner[2:])
        print("4. %s: %d reads of %d rows x %d states, windows of %d letters, W = %d, %d reads used, %d of %d candidates finite: best %.3f "
              "ms, median %.3f ms; inside decode.rescore_edits_banded_device %.3f ms (median %.3f); the rest %.3f ms"
              % (name, B, T, S, n, W, int((got.status == polish.READ_DONE).sum()), int(torch.isfinite(got.ll_edit).sum().item()),
                 int(got.ll_edit.numel()), rbest, rmed, share, float(np.median(inner[2:])), rbest - share), flush=True)


if __name__ == "__main__":
    main()
