"""What the GPU tests of rescoring share (tests/test_gpu_rescore.py, tests/test_gpu_rescore_edges.py): the calls of
decode.rescore_edits_batch and of the C entry, the extended-precision truth and the ratio to its bound."""
import ctypes
import math

import numpy as np

from tests.gpu_util import dev, stream
from tests import forward_ref as fr

E_REF = 3.219e-15
SENTINEL = -7.25


def packed(posts):
    rows = np.concatenate(posts)
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p in posts])]).astype(np.int64)
    return rows, off


def run(posts, seqs, edits, lead=0, **kw):
    """decode.rescore_edits_batch on packed rows -> (score numpy [B], [ll numpy]).  lead: so many values (NaN) lie between the
    allocation's aligned start and the first row."""
    from sloika_amd import decode
    rows, off = packed(posts)
    if lead:
        flat = dev(np.concatenate([np.full(lead, np.nan, dtype=rows.dtype), rows.reshape(-1)]))
        assert flat.data_ptr() % 16 == 0
        on_dev = flat[lead:].view(rows.shape)
    else:
        on_dev = dev(rows)
    score, ll = decode.rescore_edits_batch(on_dev, seqs, edits, row_off=off, **kw)
    return score.cpu().numpy(), [v.cpu().numpy() for v in ll]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def exact(post, seq, blank=-1):
    hi, lo = fr.forwards_exact(post, np.asarray(seq, dtype=np.int64), full=True, blank=blank)
    return np.longdouble(hi) + np.longdouble(lo)


def ratio(got, truth):
    """|got - truth| / (E_ref max(1, |truth|)); -inf must be met exactly."""
    if not np.isfinite(truth):
        assert got == float(truth), (got, truth)
        return 0.0
    assert math.isfinite(got), (got, truth)
    return float(abs(np.longdouble(got) - truth)) / (E_REF * max(1.0, abs(float(truth))))


def raw_call(posts, seqs, cands, max_npos=None, ws_bytes=None, min_prob=None, fill=SENTINEL):
    """The C entry itself, nothing checked on the host: cands = [(pair, start, ndel, new)] -> (rc, score, ll), both pre-filled."""
    import torch
    from sloika_amd import _lib
    L = _lib.lib()
    rows, off = packed(posts)
    f32 = rows.dtype == np.float32
    nread = len(posts)
    nrow = np.array([p.shape[0] for p in posts], dtype=np.int32)
    pos = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    seq = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(1, np.int32)])
    noff = np.concatenate([[0], np.cumsum([len(c[3]) for c in cands])]).astype(np.int64)
    new = np.concatenate([np.asarray(c[3], dtype=np.int32) for c in cands] + [np.zeros(1, np.int32)])
    need = L.slk_rescore_edits_workspace_bytes(nread, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p))
    d = dict(rows=dev(rows), off=dev(off[:nread].copy()), nrow=dev(nrow), seq=dev(seq), pos=dev(pos),
             pair=dev(np.array([c[0] for c in cands] + [0], dtype=np.int32)), start=dev(np.array([c[1] for c in cands] + [0], dtype=np.int32)),
             ndel=dev(np.array([c[2] for c in cands] + [0], dtype=np.int32)), noff=dev(noff), new=dev(new))
    score = torch.full((nread,), fill, dtype=torch.float64, device="cuda")
    ll = torch.full((max(len(cands), 1),), fill, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    head = (d["rows"].data_ptr(), rows.shape[1], d["off"].data_ptr(), 1, d["nrow"].data_ptr(), rows.shape[1], d["seq"].data_ptr(),
            d["pos"].data_ptr(), nread, max(len(s) for s in seqs) if max_npos is None else max_npos, rows.shape[1] - 1)
    tail = (d["pair"].data_ptr(), d["start"].data_ptr(), d["ndel"].data_ptr(), d["noff"].data_ptr(), d["new"].data_ptr(), len(cands),
            score.data_ptr(), ll.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, stream())
    if f32:
        rc = L.slk_rescore_edits_batch_f32(*head, float(min_prob or 0.0), *tail)
    else:
        rc = L.slk_rescore_edits_batch_f64(*head, *tail)
    torch.cuda.synchronize()
    return rc, score.cpu().numpy(), ll.cpu().numpy()[:len(cands)], need
