#!/usr/bin/env python3
"""Time banded rescoring (csrc/rescore_band.hip, design/rescore_band.md 7), kernels alternating in one process as
tools/rescore_edits_time.py does: best and median of --windows windows of --launches launches after two untimed windows.

    python tools/rescore_band_time.py --case reads    (a) whole reads: 64 pairs of 20 000 x 1025 float32 rows, 10 000 positions, W = 512,
                                                      every single-letter edit at kmer_len = 5: the whole entry, the lattice-only part,
                                                      ns per candidate, ps per candidate and row walked
    python tools/rescore_band_time.py --case chunks   (b) the chunk shape of design/rescore_edits.md 7 (1024 pairs, 800 x 1025, 400
                                                      positions) banded at W = 512 with lo all 0, beside the dense entry: what the
                                                      band's bookkeeping costs where it buys nothing

The posterior is random, in the network layout, blank = 0, min_prob = 1e-5; every pair carries the same draft, the band's centre is the
straight line from the first state to the last, the candidates are sorted by start.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def letter_edit_states(draft, k):
    """(start, ndel, new states) of every single-letter edit of `draft`, from the 2 k letters round it (a thousand times cheaper than
    spelling every edited string out; in a homopolymer run the edit may sit elsewhere in the run than bio.edit_states puts it)."""
    from sloika_amd import bio
    n = len(draft)
    out = []
    for p in range(n + 1):
        lo, hi = max(0, p - k), min(n, p + k + 1)
        old = bio.seq_to_states(draft[lo:hi], k)
        texts = []
        if p < n:
            texts += [draft[lo:p] + c + draft[p + 1:hi] for c in 'ACGT' if c != draft[p]] + [draft[lo:p] + draft[p + 1:hi]]
        texts += [draft[lo:p] + c + draft[p:hi] for c in 'ACGT']
        for t in texts:
            a, d, new = bio.edit_states(old, bio.seq_to_states(t, k))
            out.append((lo + a, d, new))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("reads", "chunks"), default="reads")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--letters", type=int, default=None)
    ap.add_argument("--states", type=int, default=1025)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--kmer", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    a = ap.parse_args()
    reads = a.case == "reads"
    B = a.pairs or (64 if reads else 1024)
    T = a.rows or (20000 if reads else 800)
    letters = a.letters or (10004 if reads else 404)
    S, W, k = a.states, a.width, a.kmer
    import torch
    from sloika_amd import _lib, bio, polish, device as D
    dev = D.device()
    L = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(7)
    post = torch.rand((T, B, S), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    rs = np.random.RandomState(7)
    draft = ''.join('ACGT'[i] for i in rs.randint(0, 4, size=letters))
    cols = polish.state_columns(bio.seq_to_states(draft, k), 0, S)
    P = len(cols)
    trip = sorted(letter_edit_states(draft, k), key=lambda e: e[0])
    n = len(trip)
    start = np.array([e[0] for e in trip], dtype=np.int32)
    ndel = np.array([e[1] for e in trip], dtype=np.int32)
    nnew = np.array([len(e[2]) for e in trip], dtype=np.int64)
    new = polish.state_columns(np.concatenate([np.asarray(e[2], dtype=np.int64) for e in trip]), 0, S).astype(np.int32)
    if reads:
        center = np.round(np.arange(T + 1) * (P / float(T))).astype(np.int64)
        lo_h = np.maximum.accumulate(np.clip(center - W // 2, 0, max(0, P + 1 - W))).astype(np.int32)
    else:
        lo_h = np.zeros(T + 1, dtype=np.int32)
    assert lo_h[0] == 0 and lo_h[-1] + W > P
    # the rows a workgroup of 256 sorted candidates walks: from the first row of its first column to the last of its last
    t0 = np.searchsorted(lo_h, start.astype(np.int64) - W, side="right")
    cb = start.astype(np.int64) + ndel + 1
    tend = np.where(cb <= P, np.searchsorted(lo_h, cb, side="right") - 1, T)
    walked = sum(int(max(tend[i:i + 256].max() - t0[i:i + 256].min(), 0)) * min(256, n - i) for i in range(0, n, 256))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    cand_pair = up(np.repeat(np.arange(B, dtype=np.int32), n))
    cand_start, cand_ndel = up(np.tile(start, B)), up(np.tile(ndel, B))
    cand_off = up(np.concatenate([[0], np.cumsum(np.tile(nnew, B))]).astype(np.int64))
    cand_new = up(np.tile(new, B))
    ncand = B * n
    seq = up(np.tile(cols.astype(np.int32), B))
    pos_h = np.arange(B + 1, dtype=np.int64) * P
    nrow_h = np.full(B, T, dtype=np.int32)
    pos_off, nrow, row_off = up(pos_h), up(nrow_h), torch.arange(B, dtype=torch.int64).to(dev)
    band_lo, band_off = up(np.tile(lo_h, B)), up(np.arange(B + 1, dtype=np.int64) * (T + 1))
    score = torch.empty(B, dtype=torch.float64, device=dev)
    ll = torch.empty(ncand, dtype=torch.float64, device=dev)
    host = lambda x: x.ctypes.data_as(ctypes.c_void_p)                        # noqa: E731
    need = int(L.slk_rescore_edits_banded_workspace_bytes(B, host(nrow_h), W))
    need_dense = 0 if reads else int(L.slk_rescore_edits_workspace_bytes(B, host(nrow_h), host(pos_h)))
    ws = torch.empty(max(need, need_dense), dtype=torch.uint8, device=dev)
    stream = D.stream_ptr()
    head = (post.data_ptr(), S, row_off.data_ptr(), B, nrow.data_ptr(), S, seq.data_ptr(), pos_off.data_ptr(), B)
    cands = (cand_pair.data_ptr(), cand_start.data_ptr(), cand_ndel.data_ptr(), cand_off.data_ptr(), cand_new.data_ptr())

    def banded(count):
        return lambda: _lib.check(L.slk_rescore_edits_banded_batch_f32(*head, 0, 1e-5, band_lo.data_ptr(), band_off.data_ptr(), W, *cands,
                                                                       count, score.data_ptr(), ll.data_ptr(), ws.data_ptr(), need,
                                                                       stream), "banded")

    def dense(count):
        return lambda: _lib.check(L.slk_rescore_edits_batch_f32(*head, P, 0, 1e-5, *cands, count, score.data_ptr(), ll.data_ptr(),
                                                                ws.data_ptr(), need_dense, stream), "dense")

    kernels = [("banded", banded(ncand)), ("banded, lattices only", banded(0))]
    if not reads:
        kernels += [("dense", dense(ncand)), ("dense, lattices only", dense(0))]
    times = [[] for _ in kernels]
    kept = {}
    for w in range(-2, a.windows):
        for i, (label, launch) in enumerate(kernels):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            if w >= 0:
                times[i].append(e0.elapsed_time(e1) / a.launches)
            if w == 0 and "only" not in label:
                kept[label] = (ll.cpu().numpy().copy(), score.cpu().numpy().copy())
    print("case %s: pairs %d  rows %d  states %d  positions %d  width %d  candidates %d per pair, %d in all; workspace %.2f GB; %d windows "
          "of %d launches, kernels alternating:" % (a.case, B, T, S, P, W, n, ncand, need / 1e9, a.windows, a.launches))
    best = {}
    for (label, _), t in zip(kernels, times):
        best[label] = min(t)
        print("  %-24s best %9.3f ms  median %9.3f ms" % (label, min(t), float(np.median(t))), flush=True)
        print("      windows (ms):", " ".join("%.3f" % v for v in t), flush=True)
    for name in ("banded", "dense"):
        if name in best:
            cand_ms = best[name] - best[name + ", lattices only"]
            rows_walked = walked * B if name == "banded" else ncand * T
            print("  %s: candidate kernel's share %.3f ms: %.2f ns per candidate, %.1f ps per candidate and row walked (%.0f rows per "
                  "candidate); lattices %.3f ms" % (name, cand_ms, cand_ms * 1e6 / ncand, cand_ms * 1e9 / rows_walked,
                                                    rows_walked / float(ncand), best[name + ", lattices only"]))
    got = kept["banded"]
    print("  banded ll_edit: finite %d of %d; scores finite %d of %d" % (int(np.isfinite(got[0]).sum()), ncand,
                                                                          int(np.isfinite(got[1]).sum()), B))
    if "dense" in kept:
        print("  banded / dense: %.3f (whole entry), %.3f (lattices only); the same bits: %s"
              % (best["banded"] / best["dense"], best["banded, lattices only"] / best["dense, lattices only"],
                 got[0].tobytes() == kept["dense"][0].tobytes() and got[1].tobytes() == kept["dense"][1].tobytes()))


if __name__ == "__main__":
    main()
