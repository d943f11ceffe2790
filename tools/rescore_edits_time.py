#!/usr/bin/env python3
"""Time the rescoring of edited sequences (csrc/rescore_edits.hip, design/rescore_edits.md) on a batch of chunks: every single-letter
edit of a draft under every pair, beside the two yardsticks of existing code on the same shapes in the same process.

    python tools/rescore_edits_time.py [--pairs 1024] [--rows 800] [--states 1025] [--letters 404] [--kmer 5] [--windows 7] [--launches 5]

The posterior is the one tools/forward_score_time.py makes: random, in the network layout [rows, pairs, states], read where it lies
with blank = 0 and min_prob = 1e-5, as pipeline.Basecaller.rescore_chunks does.  Every pair carries the same draft and all of its
single-letter edits, sorted by start.  Timed, the windows alternating after two untimed windows each:

    rescore          the whole entry: the copies to the host, the lattice kernel and the candidate kernel
    lattices only    the same entry without candidates (the difference is the candidate kernel's share)
    forward score    slk_forward_score_batch_f32 on ONE spelled-out edit per pair, the way to ask without this entry; printed with the
                     time it would take for all candidates at that rate
    forward-backward slk_forward_backward_batch_f32 on the pairs, which stores one lattice and walks the other

With the diagnostic build (tools/build_diag_lib.sh, SLOIKA_AMD_LIB) the candidate kernel that gathers its emissions from global memory
instead of staging rows in LDS is timed as well.  With --check the first pair's candidates are compared with the forward score of
the spelled-out sequences.
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
    ap.add_argument("--letters", type=int, default=404)
    ap.add_argument("--kmer", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--check", type=int, default=0, help="compare this many candidates of the first pair with the forward score")
    a = ap.parse_args()
    import torch
    from sloika_amd import _lib, bio, polish, device as D
    dev = D.device()
    L = _lib.lib()
    B, T, S = a.pairs, a.rows, a.states
    gen = torch.Generator(device=dev).manual_seed(7)
    post = torch.rand((T, B, S), generator=gen, device=dev, dtype=torch.float32)
    post.mul_(post)
    post.div_(post.sum(dim=2, keepdim=True))
    rs = np.random.RandomState(7)
    draft = ''.join('ACGT'[i] for i in rs.randint(0, 4, size=a.letters))
    cols, rows, eset = polish.draft_edits(draft, a.kmer, bio.EDIT_KINDS, 'ACGT', 0, S)
    P, n = len(cols), len(rows)
    order = np.argsort(eset.start, kind="stable")
    nnew = np.diff(eset.new_off)[order]
    new = np.concatenate([eset.new[eset.new_off[i]:eset.new_off[i + 1]] for i in order])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cand_pair = up(np.repeat(np.arange(B, dtype=np.int32), n))
    cand_start = up(np.tile(eset.start[order], B))
    cand_ndel = up(np.tile(eset.ndel[order], B))
    cand_off = up(np.concatenate([[0], np.cumsum(np.tile(nnew, B))]).astype(np.int64))
    cand_new = up(np.tile(new, B).astype(np.int32))
    ncand = B * n
    seq = up(np.tile(cols.astype(np.int32), B))
    pos_h = np.arange(B + 1, dtype=np.int64) * P
    nrow_h = np.full(B, T, dtype=np.int32)
    pos_off, nrow, row_off = up(pos_h), up(nrow_h), torch.arange(B, dtype=torch.int64).to(dev)
    # one spelled-out edit per pair for the forward score: pair b takes edit b * n // B
    spelled = [polish.state_columns(bio.seq_to_states(rows[(b * n) // B][3], a.kmer), 0, S).astype(np.int32) for b in range(B)]
    sp_pos_h = np.concatenate([[0], np.cumsum([len(s) for s in spelled])]).astype(np.int64)
    sp_seq, sp_pos = up(np.concatenate(spelled)), up(sp_pos_h)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    score_fs = torch.empty(B, dtype=torch.float64, device=dev)
    score_fb = torch.empty(B, dtype=torch.float64, device=dev)
    ll = torch.empty(ncand, dtype=torch.float64, device=dev)
    occ = torch.empty((T, B, S), dtype=torch.float32, device=dev)
    emit_row = torch.empty(B * P, dtype=torch.int32, device=dev)
    emit_prob = torch.empty(B * P, dtype=torch.float64, device=dev)
    host = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    need = int(L.slk_rescore_edits_workspace_bytes(B, host(nrow_h), host(pos_h)))
    need_fb = int(L.slk_forward_backward_workspace_bytes(B, host(nrow_h), host(pos_h)))
    ws = torch.empty(max(need, need_fb), dtype=torch.uint8, device=dev)
    stream = D.stream_ptr()
    pairs = (post.data_ptr(), S, row_off.data_ptr(), B, nrow.data_ptr(), S, seq.data_ptr(), pos_off.data_ptr(), B, P, 0)
    cands = (cand_pair.data_ptr(), cand_start.data_ptr(), cand_ndel.data_ptr(), cand_off.data_ptr(), cand_new.data_ptr())

    def rescore(count, gather=False):
        def launch():
            os.environ["SLK_DIAG_RESCORE_GATHER"] = "1" if gather else "0"
            _lib.check(L.slk_rescore_edits_batch_f32(*pairs, 1e-5, *cands, count, score.data_ptr(), ll.data_ptr(), ws.data_ptr(), need,
                                                     stream), "rescore")
        return launch

    kernels = [("rescore", rescore(ncand)), ("lattices only", rescore(0)),
               ("forward score", lambda: _lib.check(L.slk_forward_score_batch_f32(
                   post.data_ptr(), S, row_off.data_ptr(), B, nrow.data_ptr(), S, sp_seq.data_ptr(), sp_pos.data_ptr(), B, P + 1, 0, 1, 1e-5,
                   score_fs.data_ptr(), stream), "forward score")),
               ("forward-backward", lambda: _lib.check(L.slk_forward_backward_batch_f32(
                   *pairs, 1, 1e-5, score_fb.data_ptr(), occ.data_ptr(), S, emit_row.data_ptr(), emit_prob.data_ptr(), ws.data_ptr(), need_fb,
                   stream), "forward-backward"))]
    if os.environ.get("SLOIKA_AMD_LIB"):
        kernels.append(("rescore, gathers", rescore(ncand, gather=True)))
    times = [[] for _ in kernels]
    kept = {}
    for w in range(-2, a.windows):                       # two untimed windows first: code objects load, the clock settles
        for k, (label, launch) in enumerate(kernels):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            if w >= 0:
                times[k].append(e0.elapsed_time(e1) / a.launches)
            if w == 0 and label.startswith("rescore"):
                kept[label] = ll.cpu().numpy().copy()
    print("pairs %d  rows %d  states %d  positions %d  candidates %d per pair, %d in all; workspace %.2f GB; %d windows of %d launches, "
          "kernels alternating:" % (B, T, S, P, n, ncand, need / 1e9, a.windows, a.launches))
    best = {}
    for (label, _), t in zip(kernels, times):
        best[label] = min(t)
        print("  %-18s best %9.3f ms  median %9.3f ms" % (label, min(t), float(np.median(t))), flush=True)
        print("      windows (ms):", " ".join("%.3f" % v for v in t), flush=True)
    cand_ms = best["rescore"] - best["lattices only"]
    print("  candidate kernel's share: %.3f ms (%.2f ns per candidate, %.1f ps per candidate and row); lattices %.3f ms"
          % (cand_ms, cand_ms * 1e6 / ncand, cand_ms * 1e9 / ncand / T, best["lattices only"]))
    per = best["forward score"] / B
    print("  forward score: %.3f us per spelled-out edit -> %.1f ms for all %d candidates: %.0f times the rescoring entry"
          % (per * 1e3, per * ncand, ncand, per * ncand / best["rescore"]))
    print("  rescore / forward-backward: %.2f (best windows)" % (best["rescore"] / best["forward-backward"]))
    if "rescore, gathers" in best:
        print("  gathers from global memory / rows staged in LDS: %.2f (whole entry); the same bits: %s"
              % (best["rescore, gathers"] / best["rescore"], kept["rescore"].tobytes() == kept["rescore, gathers"].tobytes()))
    got = kept["rescore"]
    print("  ll_edit: finite %d of %d; scores finite %d of %d" % (int(np.isfinite(got).sum()), ncand, int(torch.isfinite(score).sum()), B))
    if a.check:
        from sloika_amd import decode
        pick = np.linspace(0, n - 1, min(a.check, n)).astype(int)
        srt = [rows[order[i]] for i in pick]
        seqs = [polish.state_columns(bio.seq_to_states(r[3], a.kmer), 0, S) for r in srt]
        one = post[:, 0, :].contiguous()
        want = decode.forwards_batch(one.repeat(len(pick), 1), seqs, full=True, blank=0, min_prob=1e-5,
                                     row_off=T * np.arange(len(pick) + 1)).cpu().numpy()
        err = np.abs(got[pick] - want) / np.maximum(1.0, np.abs(want))
        print("  largest relative distance from the forward score over %d candidates of pair 0: %.3e" % (len(pick), float(err.max())))


if __name__ == "__main__":
    main()
