#!/usr/bin/env python3
"""Time the pileup kernels (csrc/pileup.hip) next to the traceback launch that feeds them, on the pair sets of tools/align_traceback_time.py:

    python tools/pileup_time.py [--sets 256x2000,4096x8000] [--errors 0.12] [--depth 30] [--repeats 3] [--limit SECONDS] [--outdir profiles]

For every pair set ONE child process (this file with --worker) under a `timeout` of its own; a set that fails, faults or runs into its
limit ends the run, nothing more is started on the GPU after it.  In that process: slk_align_local_batch_u8 (the rows),
slk_align_traceback_batch_u8 (the columns), then slk_pileup_columns_u8 (with and without normalisation), slk_pileup_count_u8 and
slk_pileup_call_u8, each once to warm up and then `repeats` times between HIP events; best of the repeats, and columns per second
for each.  The pairs have no genome: pair b is placed at position b * length / depth of a made-up one, odd pairs as '-', so that
about `depth` alignments cover a position and the count kernel's atomics meet as they would in a real pileup.  Every status must be 0
and the tables must count to the rows.  Prints one JSON line per set and writes it to OUTDIR/pileup_time_PAIRSxLENGTH.json.
Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from align_time import make_pairs  # noqa: E402
from align_traceback_time import timed  # noqa: E402


def worker(args):
    import torch
    from sloika_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    qs, refs = make_pairs(args.pairs, args.length, args.errors)
    B = len(qs)
    qlen = np.array([len(x) for x in qs], dtype=np.int32)
    rlen = np.array([len(x) for x in refs], dtype=np.int64)
    max_q, max_r = int(qlen.max()), int(rlen.max())
    qh = np.zeros((B, max_q), dtype=np.uint8)
    for b, x in enumerate(qs):
        qh[b, :len(x)] = x
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(qh).to(dev)
    ql = torch.from_numpy(qlen).to(dev)
    r = torch.from_numpy(np.concatenate(refs)).to(dev)
    roff = torch.from_numpy(np.concatenate(([0], np.cumsum(rlen))).astype(np.int64)).to(dev)
    rows_d = torch.empty((B, 9), dtype=torch.int32, device=dev)
    fwd_bytes = L.slk_align_local_workspace_bytes(B, max_q, max_r)
    fwd_ws = torch.empty(max(fwd_bytes, 8), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.slk_align_local_batch_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), B, max_q, max_r, 1, 2, 2, 1,
                                          rows_d.data_ptr(), fwd_ws.data_ptr(), fwd_bytes, stream), "align_local_batch")
    del fwd_ws
    rows = rows_d.cpu().numpy()
    ncol = np.where(rows[:, 0] > 0, rows[:, 5:9].astype(np.int64).sum(axis=1), 0)
    off = np.concatenate(([0], np.cumsum(ncol))).astype(np.int64)
    need = np.array([L.slk_align_traceback_workspace_bytes(int(w[2] - w[1]), int(w[4] - w[3]), int(w[7]), int(w[8])) if w[0] > 0 else 0
                     for w in rows], dtype=np.int64)
    wo = np.concatenate(([0], np.cumsum(need))).astype(np.int64)
    ws = torch.empty(max(int(wo[-1]), 16), dtype=torch.uint8, device=dev)
    wo_d = torch.from_numpy(wo).to(dev)
    codes = torch.empty(max(int(off[-1]), 8), dtype=torch.uint8, device=dev)
    off_d = torch.from_numpy(off).to(dev)
    tb = torch.empty(B, dtype=torch.int32, device=dev)

    def traceback():
        _lib.check(L.slk_align_traceback_batch_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), B, 1, 2, 2, 1,
                                                  rows_d.data_ptr(), codes.data_ptr(), off_d.data_ptr(), codes.numel(), ws.data_ptr(),
                                                  wo_d.data_ptr(), ws.numel(), tb.data_ptr(), stream), "align_traceback_batch")

    t_tb = timed(torch, traceback, args.repeats)
    del ws
    # a made-up genome: pair b's forward view starts at b * stride (+ its r_start), odd pairs count as '-'
    stride = max(args.length // max(args.depth, 1), 1)
    minus = (np.arange(B) % 2).astype(np.int32)
    span = (rows[:, 4] - rows[:, 3]).astype(np.int64)
    t0 = np.arange(B, dtype=np.int64) * stride + np.where(minus == 1, rlen - rows[:, 4], rows[:, 3])
    G = int((t0 + span).max()) + 1
    S = args.max_ins
    minus_d, t0_d = torch.from_numpy(minus).to(dev), torch.from_numpy(t0).to(dev)
    keep_d = torch.ones(B, dtype=torch.uint8, device=dev)
    genome = torch.from_numpy(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(5).randint(0, 4, size=G)]).to(dev)
    fcodes = torch.empty_like(codes)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.zeros((G, 8), dtype=torch.int32, device=dev)
    ins = torch.zeros((G, S, 5), dtype=torch.int32, device=dev)
    letters = torch.empty((G, 1 + S), dtype=torch.uint8, device=dev)
    nlet = torch.empty(G, dtype=torch.uint8, device=dev)
    flags = torch.empty(G, dtype=torch.uint8, device=dev)

    def columns(normalise):
        _lib.check(L.slk_pileup_columns_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), rows_d.data_ptr(),
                                           codes.data_ptr(), off_d.data_ptr(), codes.numel(), tb.data_ptr(), minus_d.data_ptr(),
                                           keep_d.data_ptr(), t0_d.data_ptr(), G, B, normalise, fcodes.data_ptr(), st.data_ptr(), stream),
                   "pileup_columns")

    def count():
        _lib.check(L.slk_pileup_count_u8(q.data_ptr(), max_q, ql.data_ptr(), roff.data_ptr(), rows_d.data_ptr(), fcodes.data_ptr(),
                                         off_d.data_ptr(), fcodes.numel(), st.data_ptr(), minus_d.data_ptr(), t0_d.data_ptr(), G, B, 0, G,
                                         S, counts.data_ptr(), ins.data_ptr(), stream), "pileup_count")

    def call():
        _lib.check(L.slk_pileup_call_u8(counts.data_ptr(), ins.data_ptr(), genome.data_ptr(), G, 0, G, S, 3, letters.data_ptr(),
                                        nlet.data_ptr(), flags.data_ptr(), stream), "pileup_call")

    t_plain = timed(torch, lambda: columns(0), args.repeats)
    plain = fcodes.clone()
    t_norm = timed(torch, lambda: columns(1), args.repeats)
    changed = int((plain != fcodes)[:int(off[-1])].sum().item())
    del plain
    t_count = timed(torch, count, args.repeats)
    launches = args.repeats + 1                                  # the tables were added to by every launch, the warm-up included
    t_call = timed(torch, call, args.repeats)
    status = st.cpu().numpy()
    cn = counts.cpu().numpy().astype(np.int64)
    done = bool((tb.cpu().numpy() == 0).all() and (status == 0).all())
    counted = bool(cn[:, :6].sum() == launches * int(span.sum()) and cn[:, 6].sum() <= launches * int(rows[:, 7].sum())
                   and cn[:, 7].sum() == launches * int((span - 1).clip(min=0).sum()))
    total = int(off[-1])
    best = dict(traceback=min(t_tb), columns_plain=min(t_plain), columns_normalised=min(t_norm), count=min(t_count), call=min(t_call))
    line = json.dumps({
        "what": "traceback launch, then the three pileup kernels, between HIP events in one process, best of repeats after a warm-up each",
        "pairs": B, "length": args.length, "errors": args.errors, "depth": args.depth, "max_ins": S, "columns": total, "positions": G,
        "columns_changed_by_normalisation": changed,
        "traceback_s": t_tb, "columns_plain_s": t_plain, "columns_normalised_s": t_norm, "count_s": t_count, "call_s": t_call,
        "best_s": best, "columns_per_s": {k: (total / v if v > 0 else None) for k, v in best.items() if k != "call"},
        "positions_per_s_call": G / best["call"] if best["call"] > 0 else None,
        "count_over_traceback": best["count"] / best["traceback"], "columns_normalised_over_traceback": best["columns_normalised"] / best["traceback"],
        "all_done": done, "tables_count_to_rows": counted, "consensus_letters": int(nlet.sum().item()),
        "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if (done and counted) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="256x2000,4096x8000")
    ap.add_argument("--errors", type=float, default=0.12)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--max-ins", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a pair set's process may take")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    for item in args.sets.split(","):
        pairs, length = (int(v) for v in item.split("x"))
        out = os.path.join(args.outdir, "pileup_time_%dx%d.json" % (pairs, length))
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", "--pairs", str(pairs),
               "--length", str(length), "--errors", str(args.errors), "--depth", str(args.depth), "--max-ins", str(args.max_ins),
               "--repeats", str(args.repeats), "--out", out]
        rc = subprocess.call(cmd)
        if rc != 0:                                              # a failure, a fault or the limit: nothing more is started on the GPU
            sys.stderr.write("pileup_time: the set %s ended with status %d; stopping\n" % (item, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
