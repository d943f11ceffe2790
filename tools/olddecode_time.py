"""Time of the batch decode of a non-transducer model (olddecode.decode_post_batch: drop-bad prepare, transition estimate, profile
Viterbi, backtrace; csrc/olddecode.hip) beside the transducer decoder (decode.viterbi_batch with prepare_post fused) on the same
shape and in the same process, the two alternating.  256 reads x 800 rows, k-mer length 5: a record, not a threshold.
    python tools/olddecode_time.py [--reads 256] [--rows 800]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import olddecode_cases as oc  # noqa: E402
from sloika_amd import _lib, decode, olddecode  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=256)
ap.add_argument("--rows", type=int, default=800)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()
_lib.require_gpu()
T, B = args.rows, args.reads
# k-mer walks as in the fixture (3 % bad rows); 16 distinct reads tiled over the batch
distinct = [oc._softmax64(oc._walk_logits(T, 5, True, np.random.RandomState(900 + i))).astype(np.float32) for i in range(16)]
post = torch.from_numpy(np.stack([distinct[b % 16] for b in range(B)], axis=1)).cuda().contiguous()
ws_old, ws_new = decode.ViterbiWorkspace(), decode.ViterbiWorkspace()


def profile():
    return olddecode.decode_post_batch(post, 5, bad=True, min_prob=1e-5, workspace=ws_old)


def transducer():
    return decode.viterbi_batch(post, 5, skip_pen=0.0, min_prob=1e-5, workspace=ws_new)


def stage(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / args.calls)
    return min(ts), float(np.median(ts))


times = {"profile": [], "transducer": []}
for fn in (profile, transducer):                                   # warm every shape
    fn()
torch.cuda.synchronize()
for _ in range(3):                                                 # alternate the two
    times["profile"].append(stage(profile))
    times["transducer"].append(stage(transducer))
scores, paths, lens = profile()
torch.cuda.synchronize()
print("shape: %d reads x %d rows, 4^5 k-mers + bad column; rows kept: %.1f %%" % (B, T, 100.0 * lens.float().mean().item() / T))
for k, v in times.items():
    print("%-11s best %.3f ms   medians %s ms per batch" % (k, min(t[0] for t in v), ", ".join("%.3f" % t[1] for t in v)))
# the parts of the profile decode
prep, kept, _ = olddecode.prepare_post_drop_bad_batch(post, 5)
tr, ltr = olddecode.estimate_transitions_batch(prep, None, kept, log=True)
parts = (("prepare (drop bad)", lambda: olddecode.prepare_post_drop_bad_batch(post, 5)),
         ("transition estimate", lambda: olddecode.estimate_transitions_batch(prep, None, kept, log=True)),
         ("viterbi + backtrace", lambda: olddecode.decode_profile_batch(prep, ltr, lengths=kept, workspace=ws_old)))
for name, fn in parts:
    print("  %-20s best %.3f ms" % (name, stage(fn)[0]))
