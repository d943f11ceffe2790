#!/usr/bin/env python3
"""Time the quality-weighted pileup kernels (csrc/pileup.hip, design/pileup.md section 9) beside the plain ones, on the pair sets of
tools/pileup_time.py:

    python tools/pileup_qual_time.py [--sets 256x2000,4096x8000] [--errors 0.12] [--depth 30] [--repeats 3] [--limit SECONDS] [--outdir profiles]

For every pair set ONE child process (this file with --worker) under a `timeout` of its own; a set that fails, faults or runs into its
limit ends the run, nothing more is started on the GPU after it.  In that process: slk_align_local_batch_u8 (the rows),
slk_align_traceback_batch_u8 (the columns; timed, as the yardstick), slk_pileup_columns_u8 (normalised) once, then on those same
columns slk_pileup_count_u8 and slk_pileup_count_qual_u8, and on their tables slk_pileup_call_u8 and slk_pileup_call_qual_u8, each
once to warm up and then `repeats` times between HIP events; best of the repeats.  The qualities are random bytes 0..59 and the weight
table is the default one (min_qual 0, qmax 60), so nearly every column adds its weight: the weighted kernel issues about twice the
atomics of the plain one.  The pairs are placed as tools/pileup_time.py places them.  Every status must be 0, the plain tables of the
two count kernels must be equal, and the weighted tables must lie between 0 and 59 times the plain ones.  Prints one JSON line per set
and writes it to OUTDIR/pileup_qual_time_PAIRSxLENGTH.json.  Needs a GPU."""
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
    from sloika_amd import _lib, genome as gn
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
    qual = torch.from_numpy(np.random.RandomState(6).randint(0, 60, size=qh.shape).astype(np.uint8)).to(dev)
    weights = torch.from_numpy(gn.quality_weights(0, 60)).to(dev)
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
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)                  # noqa: E731
    pcounts, pins = zeros(G, 8), zeros(G, S, 5)                 # the plain kernel's tables
    counts, ins, wcounts, wins = zeros(G, 8), zeros(G, S, 5), zeros(G, 8), zeros(G, S, 5)
    byts = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)                   # noqa: E731
    letters, nlet, flags, letq, posq = byts(G, 1 + S), byts(G), byts(G), byts(G, 1 + S), byts(G)
    _lib.check(L.slk_pileup_columns_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), rows_d.data_ptr(),
                                       codes.data_ptr(), off_d.data_ptr(), codes.numel(), tb.data_ptr(), minus_d.data_ptr(),
                                       keep_d.data_ptr(), t0_d.data_ptr(), G, B, 1, fcodes.data_ptr(), st.data_ptr(), stream),
               "pileup_columns")

    def count():
        _lib.check(L.slk_pileup_count_u8(q.data_ptr(), max_q, ql.data_ptr(), roff.data_ptr(), rows_d.data_ptr(), fcodes.data_ptr(),
                                         off_d.data_ptr(), fcodes.numel(), st.data_ptr(), minus_d.data_ptr(), t0_d.data_ptr(), G, B, 0, G,
                                         S, pcounts.data_ptr(), pins.data_ptr(), stream), "pileup_count")

    def count_qual():
        _lib.check(L.slk_pileup_count_qual_u8(q.data_ptr(), max_q, ql.data_ptr(), qual.data_ptr(), roff.data_ptr(), rows_d.data_ptr(),
                                              fcodes.data_ptr(), off_d.data_ptr(), fcodes.numel(), st.data_ptr(), minus_d.data_ptr(),
                                              t0_d.data_ptr(), G, B, 0, G, S, weights.data_ptr(), counts.data_ptr(), ins.data_ptr(),
                                              wcounts.data_ptr(), wins.data_ptr(), stream), "pileup_count_qual")

    def call():
        _lib.check(L.slk_pileup_call_u8(pcounts.data_ptr(), pins.data_ptr(), genome.data_ptr(), G, 0, G, S, 3, letters.data_ptr(),
                                        nlet.data_ptr(), flags.data_ptr(), stream), "pileup_call")

    def call_qual():
        _lib.check(L.slk_pileup_call_qual_u8(counts.data_ptr(), ins.data_ptr(), wcounts.data_ptr(), wins.data_ptr(), genome.data_ptr(),
                                             G, 0, G, S, 3, 60, letters.data_ptr(), nlet.data_ptr(), flags.data_ptr(),
                                             letq.data_ptr(), posq.data_ptr(), stream), "pileup_call_qual")

    # plain and weighted in turn, twice over: neither has the warmer cache or clock by its place in the order
    t_count = timed(torch, count, args.repeats)
    t_qual = timed(torch, count_qual, args.repeats)
    t_count += timed(torch, count, args.repeats)
    t_qual += timed(torch, count_qual, args.repeats)
    t_call = timed(torch, call, args.repeats)
    plain_letters = int(nlet.sum().item())
    t_call_qual = timed(torch, call_qual, args.repeats)
    status = st.cpu().numpy()
    done = bool((tb.cpu().numpy() == 0).all() and (status == 0).all())
    same = bool(torch.equal(pcounts, counts) and torch.equal(pins, ins))
    wc, cn = wcounts.to(torch.int64), counts.to(torch.int64)
    bounded = bool((wc >= 0).all().item() and (wc <= 59 * cn).all().item() and (wins.to(torch.int64) <= 59 * ins.to(torch.int64)).all().item()
                   and wc.sum().item() > 0)
    total = int(off[-1])
    best = dict(traceback=min(t_tb), count=min(t_count), count_qual=min(t_qual), call=min(t_call), call_qual=min(t_call_qual))
    line = json.dumps({
        "what": "traceback launch, then the plain and the weighted count kernel on the same normalised columns and the plain and the "
                "weighted call kernel on their tables, between HIP events in one process, best of repeats after a warm-up each",
        "pairs": B, "length": args.length, "errors": args.errors, "depth": args.depth, "max_ins": S, "columns": total, "positions": G,
        "qualities": "random bytes 0..59", "weights": "min_qual 0, qmax 60",
        "traceback_s": t_tb, "count_s": t_count, "count_qual_s": t_qual, "call_s": t_call, "call_qual_s": t_call_qual,
        "best_s": best, "columns_per_s": {k: (total / best[k] if best[k] > 0 else None) for k in ("traceback", "count", "count_qual")},
        "count_qual_over_count": best["count_qual"] / best["count"], "count_over_traceback": best["count"] / best["traceback"],
        "count_qual_over_traceback": best["count_qual"] / best["traceback"], "call_qual_over_call": best["call_qual"] / best["call"],
        "all_done": done, "plain_tables_equal": same, "weighted_tables_bounded": bounded,
        "consensus_letters_plain": plain_letters, "consensus_letters_weighted": int(nlet.sum().item()),
        "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if (done and same and bounded) else 1


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
        out = os.path.join(args.outdir, "pileup_qual_time_%dx%d.json" % (pairs, length))
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", "--pairs", str(pairs),
               "--length", str(length), "--errors", str(args.errors), "--depth", str(args.depth), "--max-ins", str(args.max_ins),
               "--repeats", str(args.repeats), "--out", out]
        rc = subprocess.call(cmd)
        if rc != 0:                                              # a failure, a fault or the limit: nothing more is started on the GPU
            sys.stderr.write("pileup_qual_time: the set %s ended with status %d; stopping\n" % (item, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
