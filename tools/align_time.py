#!/usr/bin/env python3
"""Time the local-alignment kernel (csrc/align.hip) on synthetic pairs with planted errors:

    python tools/align_time.py [--pairs 4096] [--length 8000] [--errors 0.12] [--repeats 3] [--check 2] [--out FILE]

Every reference is `length` random letters; its query is a copy with `errors` of the letters substituted, followed by an inserted letter or
deleted (a third each), so queries are about as long as references.  The pairs are uploaded once; slk_align_local_batch_u8 is launched once
to warm up (code object, clocks) and then `repeats` times between HIP events.  Cell updates = sum of len(query) * len(reference).
`check` pairs are compared with the score-only DP of tests/align_ref.py on the host.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pairs(npair, length, errors, seed=31):
    rs = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    qs, refs = [], []
    for _ in range(npair):
        code = rs.randint(0, 4, size=length)
        u = rs.uniform(size=length)
        sub, ins, dele = u < errors / 3, (u >= errors / 3) & (u < 2 * errors / 3), (u >= 2 * errors / 3) & (u < errors)
        qcode = np.where(sub, (code + rs.randint(1, 4, size=length)) % 4, code)
        count = np.where(dele, 0, np.where(ins, 2, 1))
        q = np.repeat(qcode, count)
        second = np.cumsum(count)[ins] - 1                      # the inserted letter follows the one it was copied from
        q[second] = rs.randint(0, 4, size=len(second))
        qs.append(letters[q])
        refs.append(letters[code])
    return qs, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--length", type=int, default=8000)
    ap.add_argument("--errors", type=float, default=0.12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--check", type=int, default=2)
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
    out = torch.empty((B, 9), dtype=torch.int32, device=dev)
    nbytes = L.slk_align_local_workspace_bytes(B, max_q, max_r)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(L.slk_align_local_batch_u8(q.data_ptr(), max_q, ql.data_ptr(), r.data_ptr(), roff.data_ptr(), B, max_q, max_r, 1, 2, 2,
                                              1, out.data_ptr(), ws.data_ptr(), nbytes, stream), "align_local_batch")

    launch()                                                    # warm-up
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    res = out.cpu().numpy()
    same = bool(np.array_equal(res, first))                     # every launch computes the same rows
    ok = True
    if args.check:
        from tests import align_ref
        for b in range(min(args.check, B)):
            ok = ok and int(res[b, 0]) == align_ref.score_only(qs[b].tobytes(), refs[b].tobytes())
    spans = bool((res[:, 2] - res[:, 1] == res[:, 5] + res[:, 6] + res[:, 7]).all()
                 and (res[:, 4] - res[:, 3] == res[:, 5] + res[:, 6] + res[:, 8]).all())
    cells = float((qlen.astype(np.float64) * rlen).sum())
    best = min(times)
    rows = align.samacc_rows(res, ['+'] * B, qlen)
    line = json.dumps({
        "what": "slk_align_local_batch_u8 between HIP events, best of repeats after one warm-up launch", "pairs": B,
        "length": args.length, "errors": args.errors, "pass_width": align.PASS_WIDTH, "query_letters": int(qlen.sum()),
        "reference_letters": int(rlen.sum()), "cell_updates": cells, "workspace_bytes": int(nbytes), "seconds": times,
        "best_s": best, "pairs_per_s": B / best, "cell_updates_per_s": cells / best, "repeat_launches_identical": same,
        "scores_checked": int(min(args.check, B)), "scores_ok": bool(ok), "spans_consistent": spans,
        "mean_accuracy": align.summary(rows).get("mean"), "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if (same and ok and spans) else 1


if __name__ == "__main__":
    sys.exit(main())
