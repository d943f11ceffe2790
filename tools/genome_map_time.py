#!/usr/bin/env python3
"""Time the stages of locating reads on a genome (csrc/genome_map.hip, sloika_amd/genome.py) on a synthetic run:

    python tools/genome_map_time.py [--genome 4600000] [--queries 4096] [--length 8000] [--errors 0.12] [--repeats 3] [--out FILE]

A seeded random genome in one contig; every query is a stretch of `length` letters of it with tests/align_cases.mutate's errors
(substitutions, insertions, deletions in equal parts), every other one reverse-complemented.  Between HIP events, after one warm-up
each: the index build (keys kernel + sort), the seed stage, the cut of the windows, the aligner launch on the windows -- and, beside
it, the same aligner launch on the TRUE loci (`length` letters each, reverse-complemented where the read is), so that the window's
extra columns and the seed stage read as a ratio to the alignment that has to be done anyway.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    import torch
    fn()                                                        # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return min(times), times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--length", type=int, default=8000)
    ap.add_argument("--errors", type=float, default=0.12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from sloika_amd import _lib, align, genome
    from tests import align_cases
    _lib.require_gpu()
    L = _lib.lib()
    rs = np.random.RandomState(51)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = letters[rs.randint(0, 4, size=args.genome)]
    text = g.tobytes().decode()
    at = rs.randint(0, args.genome - args.length + 1, size=args.queries)
    minus = np.arange(args.queries) % 2 == 1
    qs = []
    for b in range(args.queries):
        q = align_cases.mutate(rs, text[at[b]:at[b] + args.length], args.errors)
        qs.append(align_cases.revcomp(q) if minus[b] else q)

    build_ms, build_all, idx = timed(lambda: genome.Index([("genome", g)]), args.repeats)
    stream = torch.cuda.current_stream().cuda_stream
    q, ldq, qlen, lens, max_qlen = idx._upload(qs)
    B = len(qs)

    # the seed stage: the launch alone (its rows come to the host once, behind the timing)
    nbytes = L.slk_genome_seed_workspace_bytes(B, max_qlen, idx.G, idx.bin_width)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    seeds_d = torch.empty((B, 2, 4), dtype=torch.int32, device=q.device)

    def seed():
        _lib.check(L.slk_genome_seed_votes_u8(q.data_ptr(), ldq, qlen.data_ptr(), B, max_qlen, idx.keys.data_ptr(), idx.nvalid, idx.G,
                                              idx.k, idx.bin_width, idx.max_occ, seeds_d.data_ptr(), ws.data_ptr(), nbytes, stream),
                   "genome_seed_votes")
    seed_ms, seed_all, _ = timed(seed, args.repeats)
    seeds = seeds_d.cpu().numpy()
    seed()
    torch.cuda.synchronize()
    seeds_same = bool(np.array_equal(seeds_d.cpu().numpy(), seeds))

    # the whole map once for the placement, then its two device stages on their own
    res, strand, info = idx.map(qs)
    placed = (info['contig'] == 0) & (strand == np.where(minus, '-', '+')) & (np.abs(res[:, 3] - at) < 0.05 * args.length)
    ws0, we0 = info['window_start'], info['window_end']
    cut_ms, cut_all, (wref, woff, woff_d) = timed(lambda: idx.cut(ws0, we0, strand == '-'), args.repeats)
    true_ref, toff, toff_d = idx.cut(at, at + args.length, minus)

    def aligner(ref, off_d, max_rlen):
        nb = L.slk_align_local_workspace_bytes(B, max_qlen, max_rlen)
        wsp = torch.empty(max(nb, 8), dtype=torch.uint8, device=q.device)
        out = torch.empty((B, 9), dtype=torch.int32, device=q.device)

        def launch():
            _lib.check(L.slk_align_local_batch_u8(q.data_ptr(), ldq, qlen.data_ptr(), ref.data_ptr(), off_d.data_ptr(), B, max_qlen,
                                                  max_rlen, 1, 2, 2, 1, out.data_ptr(), wsp.data_ptr(), nb, stream), "align_local_batch")
            return out
        return launch

    win_ms, win_all, wout = timed(aligner(wref, woff_d, int((we0 - ws0).max())), args.repeats)
    true_ms, true_all, tout = timed(aligner(true_ref, toff_d, args.length), args.repeats)
    wres, tres = wout.cpu().numpy(), tout.cpu().numpy()
    line = json.dumps({
        "what": "index build, seed stage, window cut and windowed alignment between HIP events, best of repeats after one warm-up each; "
                "beside it the aligner on the true loci",
        "genome_letters": args.genome, "queries": B, "length": args.length, "errors": args.errors, "k": idx.k, "bin_width": idx.bin_width,
        "max_occ": idx.max_occ, "valid_kmers": idx.nvalid, "query_letters": int(lens.sum()),
        "index_build_ms": build_ms, "index_build_all_ms": build_all,
        "seed_ms": seed_ms, "seed_all_ms": seed_all, "seed_queries_per_s": B / (seed_ms / 1e3), "seed_workspace_bytes": int(nbytes),
        "seed_rows_identical": seeds_same,
        "cut_ms": cut_ms, "window_letters_mean": float((we0 - ws0).mean()), "window_letters_max": int((we0 - ws0).max()),
        "align_windows_ms": win_ms, "align_windows_all_ms": win_all, "align_true_loci_ms": true_ms, "align_true_loci_all_ms": true_all,
        "window_over_true": win_ms / true_ms, "seed_over_true": seed_ms / true_ms,
        "placed_on_their_locus": int(placed.sum()), "edge": int(info['edge'].sum()), "unmapped": int((info['contig'] < 0).sum()),
        "scores_equal_true_locus": int((wres[:, 0] == tres[:, 0]).sum()), "scores_above_true_locus": int((wres[:, 0] > tres[:, 0]).sum()),
        "scores_below_true_locus": int((wres[:, 0] < tres[:, 0]).sum()),
        "votes_median": float(np.median(info['votes'])), "second_max": int(info['second'].max()),
        "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if seeds_same else 1


if __name__ == "__main__":
    sys.exit(main())
