#!/usr/bin/env python3
"""Time the alignment traceback (csrc/align_traceback.hip) next to the forward pass it follows, on the pair sets of tools/align_time.py:

    python tools/align_traceback_time.py [--pairs 4096] [--length 8000] [--errors 0.12] [--repeats 3] [--workspace-limit BYTES] [--out FILE]

In one process: slk_align_local_batch_u8 (the forward launch), slk_align_traceback_batch_u8 on its rows (one launch, or consecutive
launches split at --workspace-limit bytes of traceback workspace, as align.align_batch(ops=True, workspace_limit=...) splits them) and
slk_align_error_profile_u8, each once to warm up and then `repeats` times between HIP events; best of the repeats.  Every pair's status
must be 0 and every pair's profile must count to its row (aligned pairs, insertions, deletions, and matches on the diagonal of the
A C G T block).  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from align_time import make_pairs  # noqa: E402


def timed(torch, fn, repeats):
    fn()                                                        # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--length", type=int, default=8000)
    ap.add_argument("--errors", type=float, default=0.12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workspace-limit", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from sloika_amd import _lib, align
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

    def forward():
        _lib.check(L.slk_align_local_batch_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), B, max_q, max_r, 1, 2, 2,
                                              1, rows_d.data_ptr(), fwd_ws.data_ptr(), fwd_bytes, stream), "align_local_batch")

    t_fwd = timed(torch, forward, args.repeats)
    del fwd_ws
    rows = rows_d.cpu().numpy()
    ncol = np.where(rows[:, 0] > 0, rows[:, 5:9].astype(np.int64).sum(axis=1), 0)
    off = np.concatenate(([0], np.cumsum(ncol))).astype(np.int64)
    need = np.array([L.slk_align_traceback_workspace_bytes(int(w[2] - w[1]), int(w[4] - w[3]), int(w[7]), int(w[8])) if w[0] > 0 else 0
                     for w in rows], dtype=np.int64)
    runs = align._traceback_runs(need, args.workspace_limit)
    ws_offs = [np.concatenate(([0], np.cumsum(need[lo:hi]))).astype(np.int64) for lo, hi in runs]
    ws = torch.empty(max(max(int(w[-1]) for w in ws_offs), 16), dtype=torch.uint8, device=dev)
    ws_offs_d = [torch.from_numpy(w).to(dev) for w in ws_offs]
    codes = torch.empty(max(int(off[-1]), 8), dtype=torch.uint8, device=dev)
    off_d = torch.from_numpy(off).to(dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    profile = torch.empty((B, 68), dtype=torch.int32, device=dev)

    def traceback():
        for (lo, hi), wo in zip(runs, ws_offs_d):
            _lib.check(L.slk_align_traceback_batch_u8(q[lo:hi].data_ptr(), max_q, ql[lo:hi].data_ptr(), r.data_ptr(),
                                                      roff[lo:hi + 1].data_ptr(), hi - lo, 1, 2, 2, 1, rows_d[lo:hi].data_ptr(),
                                                      codes.data_ptr(), off_d[lo:hi + 1].data_ptr(), codes.numel(), ws.data_ptr(),
                                                      wo.data_ptr(), ws.numel(), status[lo:hi].data_ptr(), stream),
                       "align_traceback_batch")

    def prof():
        _lib.check(L.slk_align_error_profile_u8(q.data_ptr(), max_q, r.data_ptr(), roff.data_ptr(), rows_d.data_ptr(), codes.data_ptr(),
                                                off_d.data_ptr(), status.data_ptr(), B, profile.data_ptr(), stream),
                   "align_error_profile")

    t_tb = timed(torch, traceback, args.repeats)
    t_pr = timed(torch, prof, args.repeats)
    st = status.cpu().numpy()
    p = profile.cpu().numpy().astype(np.int64)
    m = p[:, :36].reshape(B, 6, 6)
    done = bool((st == 0).all())
    counts = bool((m[:, :5, :5].sum(axis=(1, 2)) == rows[:, 5] + rows[:, 6]).all() and (m[:, :5, 5].sum(axis=1) == rows[:, 7]).all()
                  and (m[:, 5, :5].sum(axis=1) == rows[:, 8]).all()
                  and (m[:, :4, :4].diagonal(axis1=1, axis2=2).sum(axis=1) == rows[:, 5]).all()
                  and (p[:, 36:52].sum(axis=1) <= rows[:, 7]).all() and (p[:, 52:68].sum(axis=1) <= rows[:, 8]).all())
    band = rows[:, 7] + rows[:, 8] + 1
    f, t, pr = min(t_fwd), min(t_tb), min(t_pr)
    s = align.error_summary(p)
    line = json.dumps({
        "what": "forward, traceback and error-profile launches between HIP events in one process, best of repeats after a warm-up each",
        "pairs": B, "length": args.length, "errors": args.errors, "band_mean": float(band.mean()), "band_max": int(band.max()),
        "max_band": int(L.slk_align_traceback_max_band()), "columns": int(off[-1]), "forward_workspace_bytes": int(fwd_bytes),
        "traceback_workspace_bytes": int(need.sum()), "traceback_launches": len(runs),
        "traceback_workspace_bytes_largest_launch": int(max(int(w[-1]) for w in ws_offs)), "forward_s": t_fwd, "traceback_s": t_tb,
        "profile_s": t_pr, "forward_best_s": f, "traceback_best_s": t, "profile_best_s": pr, "traceback_over_forward": t / f,
        "traceback_plus_profile_over_forward": (t + pr) / f, "all_done": done, "profiles_count_to_rows": counts,
        "mismatch_rate": s['mismatch_rate'], "insertion_rate": s['insertion_rate'], "deletion_rate": s['deletion_rate'],
        "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if (done and counts) else 1


if __name__ == "__main__":
    sys.exit(main())
