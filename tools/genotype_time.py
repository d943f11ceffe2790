#!/usr/bin/env python3
"""Time the variant caller (csrc/genotype.hip, design/genotypes.md Time) on polish_variants_time.py's workload.  A record, not a
threshold.

    python tools/genotype_time.py [--reads 64] [--letters 10000] [--rows 20000] [--kmer 5] [--width 512]

Each figure is the best and the median of its timed repeats (--launches for figures 1 and 2, --windows for 3) after two untimed ones,
the device idle in between (torch.cuda.synchronize round every repeat, wall clock: the entries hold host round trips, which belong to
their cost):
  1. genome.Pileup.alleles of the whole genome: count, prefix sums, emit.  The tables are written by hand: a depth of 8 on the
     reference letter everywhere, and at one position in 64 each a minority substitution, a deleted letter and an inserted letter;
  2. polish.variant_genotype_likelihoods for the candidates polish.variant_edits makes of the repeat proposals for --reads windows,
     torch's two stable sorts included, and the host half (polish.call_genotypes) beside it;
  3. a whole polish.call_variants(variants='repeats') beside polish.rescore_variants('repeats') on the same reads, each with the share
     of it spent inside decode.rescore_edits_banded_device (the scoring kernels, unchanged).  The reads are error-free, so the pileup
     proposes nothing and both score the same variants: the difference is the pileup, the alleles, the genotypes and the VCF rows.

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
    ap.add_argument("--windows", type=int, default=5, help="timed repeats of the whole calls")
    ap.add_argument("--launches", type=int, default=100, help="timed repeats of figures 1 and 2")
    a = ap.parse_args()
    import torch
    from sloika_amd import align, bio, decode, genome as GM, polish, device as D
    dev = D.device()
    B, n, T, k, W = a.reads, a.letters, a.rows, a.kmer, a.width
    S = 4 ** k + 1
    rs = np.random.RandomState(7)
    step = max(n // 8, 1)
    G = n + step * (B - 1)
    text = ''.join('ACGT'[i] for i in rs.randint(0, 4, size=G))
    letters = np.frombuffer(text.encode('ascii'), dtype=np.uint8).copy()
    genome = torch.from_numpy(letters).to(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    w0 = np.arange(B, dtype=np.int64) * step
    minus = (np.arange(B) % 2).astype(np.int32)
    win = (up(np.zeros(B, dtype=np.int64)), up(w0), up(w0 + n), up(minus))
    index = types.SimpleNamespace(offsets=np.array([0, G], dtype=np.int64), G=G, genome=genome, names=["g"], lengths=np.array([G]))

    pile = GM.Pileup(index, max_ins=4)
    digit = np.array([{'A': 0, 'C': 1, 'G': 2, 'T': 3}[ch] for ch in text])
    counts = np.zeros((G, 8), dtype=np.int32)
    counts[np.arange(G), digit] = 8
    counts[:, 7] = 8
    counts[np.arange(0, G, 64), (digit[::64] + 1) % 4] = 3
    counts[np.arange(21, G, 64), 5] = 3
    ins = np.zeros((G, 4, 5), dtype=np.int32)
    ins[np.arange(42, G, 64), 0, 2] = 3
    pile.counts_dev.copy_(up(counts))
    pile.ins_dev.copy_(up(ins))
    best, med, al = timed(lambda: pile.alleles(k), a.launches)
    print("1. Pileup.alleles: %d letters, kmer_len %d: %d proposals, %d alt letters: best %.3f ms, median %.3f ms"
          % (G, k, al.V, al.A, best, med), flush=True)
    pile.counts_dev.zero_()
    pile.ins_dev.zero_()

    vs = polish.repeat_variants(index, k)
    c = polish.variant_edits(genome, vs.contig_off, *win, vs, k, 0, 2 * k)
    gen = torch.Generator(device=dev).manual_seed(7)
    ll = torch.randn(c.ncand, generator=gen, device=dev, dtype=torch.float64)
    score = torch.randn(B, generator=gen, device=dev, dtype=torch.float64)
    gbest, gmed, (gl, cnt) = timed(lambda: polish.variant_genotype_likelihoods(score, ll, c.cand_pair, c.cand_var, vs.V), a.launches)
    sbest, smed, _ = timed(lambda: polish.sum_variant_gains(score, ll, c.cand_pair, c.cand_var, win[3], vs.V), a.launches)
    gl_h, cnt_h = gl.cpu().numpy(), cnt.cpu().numpy()
    hbest, hmed, _ = timed(lambda: polish.call_genotypes(gl_h, cnt_h), a.launches)
    print("2. variant_genotype_likelihoods: %d candidates on %d variants: best %.3f ms, median %.3f ms (the sort by (variant, read) "
          "included; sum_variant_gains beside it: best %.3f ms, median %.3f ms); call_genotypes on the host: best %.3f ms, median %.3f ms"
          % (c.ncand, vs.V, gbest, gmed, sbest, smed, hbest, hmed), flush=True)

    post = torch.rand((T, B, S), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    nk = n - k + 1
    paths, mrow = np.zeros((B, nk), dtype=np.int32), np.zeros((B, nk), dtype=np.int32)
    q = np.zeros((B, n), dtype=np.uint8)
    for b in range(B):
        s = text[w0[b]:w0[b] + n]
        s = ''.join({'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}[ch] for ch in reversed(s)) if minus[b] else s
        q[b] = np.frombuffer(s.encode('ascii'), dtype=np.uint8)
        paths[b] = bio.seq_to_states(s, k)
        mrow[b] = (np.arange(nk, dtype=np.int64) * T) // nk
    rows = np.tile(np.array([n, 0, n, 0, n, n, 0, 0, 0], dtype=np.int32), (B, 1))
    off = np.arange(B + 1, dtype=np.int64) * n
    part = (up(q.reshape(-1)), up(off), up(rows), torch.zeros(B, dtype=torch.int32, device=dev))
    ops = align.Ops(up(q), n, up(np.full(B, n, dtype=np.int32)), [part], rows, torch.zeros(B * n, dtype=torch.uint8, device=dev), off,
                    up(off), np.zeros(B, dtype=np.int32))
    info = {'contig': np.zeros(B, dtype=np.int64), 'window_start': w0, 'window_end': w0 + n}
    strand = np.where(minus, '-', '+')
    call = (up(paths), up(np.full(B, nk, dtype=np.int32)), up(mrow))
    steps = up(np.full(B, T, dtype=np.int32))
    entry = decode.rescore_edits_banded_device

    def whole():
        calls = polish.call_variants(post, steps, call[0], call[1], call[2], index, rows, strand, info, ops, k, variants='repeats', width=W,
                                     min_prob=1e-5)
        calls.nrows = len(calls.rows())
        return calls

    for name, fn in (("rescore_variants('repeats')", lambda: polish.rescore_variants(post, steps, call[0], call[1], call[2], index, rows,
                                                                                     strand, info, ops, k, 'repeats', width=W, min_prob=1e-5)),
                     ("call_variants(variants='repeats')", whole)):
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
        more = ""
        if hasattr(got, 'rescored'):
            more = "; %d alleles of the pileup (depth %d at its middle), %d variants genotyped, %d non-reference rows" % (
                len(got.variants) - vs.V, int(got.pileup.counts_dev[G // 2, :6].sum().item()), len(got.variants), got.nrows)
            got = got.rescored
        print("3. %s: %d reads of %d rows x %d states, windows of %d letters, W = %d, %d reads used, %d of %d candidates finite: best %.3f "
              "ms, median %.3f ms; inside decode.rescore_edits_banded_device %.3f ms (median %.3f), %.1f %% of it; the rest %.3f ms%s"
              % (name, B, T, S, n, W, int((got.status == polish.READ_DONE).sum()), int(torch.isfinite(got.ll_edit).sum().item()),
                 int(got.ll_edit.numel()), rbest, rmed, share, float(np.median(inner[2:])), 100.0 * share / rbest, rbest - share, more),
              flush=True)


if __name__ == "__main__":
    main()
