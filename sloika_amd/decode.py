"""decode API of the reference (sloika/decode.py) on the HIP kernels of csrc/decode.hip.

    argmax(post, zero_is_blank=True)                       decode.py:5-18
    prepare_post(post, min_prob=1e-5, drop_bad=False)      decode.py:21-36
    viterbi(post, klen, skip_pen=0.0, log=False, nbase=4)  decode.py:39-93      -> (score, [states])
    viterbi_batch(post[T,B,S], ...)                        batched extension    -> (scores[B], paths[B,T], lens[B])
    score(post, seq, full=False)                           decode.py:96-105
    forwards(post, seq, full=False)                        decode.py:108-139    -> float64 (csrc/forward_score.hip)
    forwards_batch(post[T,B,S] | rows + row_off, seqs)     batched extension    -> scores[B] float64, on the device
    forwards_backwards(post, seq, full=False)              the backward half    -> (score, occ, emit_row, emit_prob)
    forwards_backwards_batch(post | rows + row_off, seqs)  (csrc/forward_backward.hip, design/forward_backward.md)
    rescore_edits_batch(post | rows + row_off, seqs, edits) the full forward score of every EDITED sequence from one stored pair of
                                                           lattices (csrc/rescore_edits.hip, design/rescore_edits.md; polish.py)
    viterbi_marginals_batch(post[T,B,S], klen, ...)        the decoder's sum-product twin: state marginals, log Z, a confidence per
                                                           called position (csrc/lattice_marginals.hip, design/lattice_marginals.md)

Inputs may be numpy arrays or device tensors; float32 arithmetic (the network's dtype).  float64 input is
converted to float32 first -- unlike numpy, which would then decode in float64.  The forward score is the exception:
it runs in float64 on float32 or float64 rows, as numpy does.
forwards_transpose / backwards_transpose (decode.py:142-211) have no counterpart: design/forward_score.md.
"""
import numpy as np

from . import _lib, profiler
from . import variables as sv


def _dev(x):
    from . import device as D
    return D.to_dev(x)


def argmax(post, zero_is_blank=True):
    """Argmax decoding of simple transducer (decode.py:5-18): 1D array of called states."""
    import torch
    from . import device as D
    pd = _dev(post)
    assert pd.dim() == 2
    T, S = pd.shape
    path = torch.empty((1, T), dtype=torch.int32, device=pd.device)
    n = torch.empty(1, dtype=torch.int32, device=pd.device)
    _lib.check(_lib.lib().slk_argmax_decode_f32(pd.data_ptr(), T, 1, S, int(bool(zero_is_blank)), path.data_ptr(),
                                                n.data_ptr(), D.stream_ptr()), "decode.argmax")
    return path[0, : int(n.item())].cpu().numpy().astype(np.int64)


def prepare_post(post, min_prob=1e-5, drop_bad=False):
    """Sanitised posterior matrix for decoding (decode.py:21-36): [T,1,S] -> [T,S]."""
    import torch
    from . import device as D
    if drop_bad:
        # decode.py:31-35: the rows called bad (first arg-max in column 0) and the bad column leave, the rest is renormalised
        from . import olddecode
        if len(post.shape) != 3 or post.shape[1] != 1:
            raise ValueError("prepare_post expects a [time, 1, state] posterior (np.squeeze(axis=1), decode.py:30)")
        out, kept, _ = olddecode.prepare_post_drop_bad_batch(post, olddecode.klen_of(post.shape[2] - 1), min_prob=min_prob)
        return D.like_input(out[: int(kept[0].item()), 0, :], post)
    pd = _dev(post)
    if pd.dim() != 3 or pd.shape[1] != 1:
        raise ValueError("prepare_post expects a [time, 1, state] posterior (np.squeeze(axis=1), decode.py:30)")
    pd = pd[:, 0, :].contiguous()
    out = torch.empty_like(pd)
    _lib.check(_lib.lib().slk_prepare_post_f32(pd.data_ptr(), out.data_ptr(), pd.numel(), float(min_prob),
                                               D.stream_ptr()), "decode.prepare_post")
    return D.like_input(out, post)


class ViterbiWorkspace(object):
    """Reusable device buffers for viterbi_batch (traceback bytes dominate: T*B*nkmer)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        import torch
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = None
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


def viterbi_batch(post, klen, skip_pen=0.0, log=False, nbase=4, min_prob=None, workspace=None):
    """Batched decode.viterbi over the batch axis of a [T, B, nstate] posterior.

    min_prob: if given, decode.prepare_post's transform is applied first (fused), i.e. `post` is the raw
    network output as in basecall.decode_post (sloika/basecall.py:26-51).
    Returns device tensors (scores float32 [B], paths int32 [B, T] left aligned and -1 padded, lens int32 [B]).
    """
    import torch
    from . import device as D
    pd = _dev(post)
    if pd.dim() != 3:
        raise ValueError("viterbi_batch expects [time, batch, state]")
    T, B, S = pd.shape
    if klen < 3:
        raise ValueError("Kmer not long enough to apply Viterbi with skips")          # decode.py:50
    if sv.nstate(klen, transducer=True, nbase=nbase) != S:
        raise ValueError("posterior has %d states, klen=%d nbase=%d needs %d" % (S, klen, nbase, sv.nstate(klen, nbase=nbase)))
    L = _lib.lib()
    mode = _lib.POST_LOG if log else (_lib.POST_RAW if min_prob is not None else _lib.POST_PLAIN)
    nbytes = L.slk_viterbi_kmer_workspace_bytes(T, B, nbase, klen)
    if nbytes == 0:
        raise ValueError("unsupported klen/nbase for the Viterbi kernel")
    ws = (workspace or ViterbiWorkspace()).get(nbytes, pd.device)
    scores = D.scratch(B, torch.float32, pd.device, result=True)
    paths = D.scratch((B, T), torch.int32, pd.device, result=True)
    lens = D.scratch(B, torch.int32, pd.device, result=True)
    nk = nbase ** klen
    with profiler.region("viterbi", 0.0, float(T) * B * (4.0 * S + 2.0 * nk)):
        rc = L.slk_viterbi_kmer_f32(pd.data_ptr(), T, B, nbase, klen, float(skip_pen), mode,
                                    float(min_prob if min_prob is not None else 0.0), ws.data_ptr(), nbytes,
                                    scores.data_ptr(), paths.data_ptr(), lens.data_ptr(), D.stream_ptr())
    _lib.check(rc, "decode.viterbi")
    return scores, paths, lens


def marginals_rows_per_checkpoint(checkpoint):
    """The `every` argument of slk_viterbi_marginals_ckpt_f32 for viterbi_marginals_batch's `checkpoint`: None for None (the stored-row
    kernel), 0 for True (the kernel's own choice), else the integer K >= 1."""
    if checkpoint is None:
        return None
    if checkpoint is True:
        return 0
    if checkpoint is False or int(checkpoint) != checkpoint or int(checkpoint) < 1:
        raise ValueError("checkpoint is None, True or the rows per checkpoint (an integer >= 1)")
    return int(checkpoint)


def marginals_default_rows(nbase, klen):
    """The rows per checkpoint slk_viterbi_marginals_ckpt_f32 takes for every = 0: what 36 KiB of LDS hold of 9 nbase^klen bytes per
    row, at most 64 (csrc/lattice_marginals.hip, lmc_every; design/lattice_marginals.md 8)."""
    return max(1, min(64, (36 * 1024) // (9 * nbase ** klen)))


def marginals_workspace_bytes(T, B, nbase, klen, checkpoint=None):
    """Bytes of workspace one launch of viterbi_marginals_batch takes for B chunks of T rows (0 for a shape the kernels refuse)."""
    L = _lib.lib()
    every = marginals_rows_per_checkpoint(checkpoint)
    if every is None:
        return int(L.slk_viterbi_marginals_workspace_bytes(T, B, nbase, klen))
    return int(L.slk_viterbi_marginals_ckpt_workspace_bytes(T, B, nbase, klen, every))


def viterbi_marginals_batch(post, klen, skip_pen=0.0, nbase=4, min_prob=1e-5, lengths=None, gamma=False, workspace_limit=None,
                            checkpoint=None):
    """viterbi_batch and, over the same lattice, the sum over ALL its paths (csrc/lattice_marginals.hip,
    design/lattice_marginals.md): how much of the total likelihood passes through each state at each row, and how sure the called
    path is of each of its positions.

    post: [T, B, nbase^klen + 1] float32 (numpy or device tensor), the raw network output; min_prob: decode.prepare_post's floor,
    applied first (None: `post` is taken as it is).  lengths: None, or per chunk the rows it owns (host integers or an int32 device
    tensor), clamped to 1 .. T.  nbase 4 or 5, klen >= 3, at most 1024 k-mers.
    -> (scores float32 [B], paths int32 [B, T], lens int32 [B]: the bits of viterbi_batch;
        move_row int32 [B, T]: the row at which the path enters each of its states (-1 behind lens[b]);
        conf float64 [B, T]: per position the largest marginal of its state over the rows it dwells on (0 behind lens[b]);
        logz float64 [B]: the log of the summed weight of all paths;
        and with gamma=True, gamma float32 [T, B, nbase^klen]: the marginals, every row of a chunk summing to 1), all on the device.
    The forward rows of a launch live in a workspace of 9 nbase^klen + 20 bytes per row and chunk; the batch runs as consecutive
    launches whose workspace stays within `workspace_limit` bytes (default transducer.WORKSPACE_LIMIT; a chunk's results do not depend
    on the split).  A chunk that needs more on its own raises ValueError.

    checkpoint: None runs slk_viterbi_marginals_f32 as above.  True, or an integer K >= 1, runs slk_viterbi_marginals_ckpt_f32, which
    keeps the forward state of every K-th row only (True: the kernel's own K for nbase^klen) and recomputes the rows between in LDS:
    about 13 nbase^klen / K + 20 bytes per row and chunk, which is then what `workspace_limit` splits by.  Every output has the same
    bits whatever `checkpoint` is."""
    import torch
    from . import device as D
    from . import transducer
    pd = _dev(post)
    if pd.dim() != 3:
        raise ValueError("viterbi_marginals_batch expects [time, batch, state]")
    every = marginals_rows_per_checkpoint(checkpoint)
    T, B, S = pd.shape
    if klen < 3:
        raise ValueError("Kmer not long enough to apply Viterbi with skips")          # decode.py:50
    if sv.nstate(klen, transducer=True, nbase=nbase) != S:
        raise ValueError("posterior has %d states, klen=%d nbase=%d needs %d" % (S, klen, nbase, sv.nstate(klen, nbase=nbase)))
    if min_prob is not None and not 0.0 <= float(min_prob) < 1.0:
        raise ValueError("min_prob must lie in [0, 1)")
    L = _lib.lib()

    def need(n):
        return marginals_workspace_bytes(T, n, nbase, klen, checkpoint)

    alone = need(1) if T >= 1 else 0
    if T < 1 or B < 1 or alone == 0:
        raise ValueError("the lattice marginals take nbase 4 or 5, klen >= 3 and at most 1024 k-mers")
    limit = transducer.WORKSPACE_LIMIT if workspace_limit is None else int(workspace_limit)
    if alone > limit:
        raise ValueError("a chunk needs %d bytes of workspace, above the workspace_limit of %d" % (alone, limit))
    lens_d = None
    if lengths is not None:
        lens_d = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths, dtype=np.int32))
        if lens_d.numel() != B:
            raise ValueError("lengths needs one entry per chunk")
        lens_d = lens_d.to(device=pd.device, dtype=torch.int32).contiguous()
    nk = nbase ** klen
    dev = pd.device
    scores = D.scratch(B, torch.float32, dev, result=True)
    paths = D.scratch((B, T), torch.int32, dev, result=True)
    lens = D.scratch(B, torch.int32, dev, result=True)
    move_row = D.scratch((B, T), torch.int32, dev, result=True)
    conf = D.scratch((B, T), torch.float64, dev, result=True)
    logz = D.scratch(B, torch.float64, dev, result=True)
    gam = D.scratch((T, B, nk), torch.float32, dev, result=True) if gamma else None
    per = max(1, min(B, limit // alone))                         # (the size is a multiple of 256 per call, never more than B * alone)
    runs = [(lo, min(lo + per, B)) for lo in range(0, B, per)]
    ws = torch.empty(need(runs[0][1] - runs[0][0]), dtype=torch.uint8, device=dev)
    mode = _lib.POST_RAW if min_prob is not None else _lib.POST_PLAIN
    with profiler.region("lattice_marginals", 20.0 * T * B * nk, float(T) * B * (8.0 * S + 18.0 * nk)):
        for lo, hi in runs:
            n = hi - lo
            whole = n == B
            sub = pd if whole else pd[:, lo:hi].contiguous()
            g = gam if whole or gam is None else torch.empty((T, n, nk), dtype=torch.float32, device=dev)
            head = (sub.data_ptr(), T, n, nbase, klen, float(skip_pen), mode, float(min_prob if min_prob is not None else 0.0),
                    None if lens_d is None else lens_d[lo:hi].data_ptr())
            tail = (ws.data_ptr(), need(n), scores[lo:hi].data_ptr(), paths[lo:hi].data_ptr(), lens[lo:hi].data_ptr(),
                    move_row[lo:hi].data_ptr(), conf[lo:hi].data_ptr(), logz[lo:hi].data_ptr(), D.ptr(g), D.stream_ptr())
            if every is None:
                rc = L.slk_viterbi_marginals_f32(*(head + tail))
            else:
                rc = L.slk_viterbi_marginals_ckpt_f32(*(head + (every,) + tail))
            _lib.check(rc, "decode.viterbi_marginals")
            if g is not None and not whole:
                gam[:, lo:hi] = g
    return (scores, paths, lens, move_row, conf, logz) + ((gam,) if gamma else ())


def viterbi_logits_batch(logits, stats, klen, T, B, ld=None, skip_pen=0.0, nbase=4, min_prob=1e-5, workspace=None,
                         lengths=None):
    """basecall.decode_post over the batch axis, fed with the Softmax layer's LOGITS (rows (t,b) of nstate floats, `ld`
    floats apart) and their row statistics (layers.Softmax.logits_and_stats): softmax, prepare_post, log and Viterbi in one pass over the logits.
    Bit-identical to viterbi_batch(softmax(logits), min_prob=min_prob).  `lengths`: optional int32 device tensor [B] for a
    ragged batch (chunk b decoded over its first lengths[b] steps only)."""
    import torch
    from . import device as D
    if klen < 3:
        raise ValueError("Kmer not long enough to apply Viterbi with skips")
    S = sv.nstate(klen, transducer=True, nbase=nbase)
    ld = S if ld is None else ld
    if ld < S or logits.numel() < T * B * ld:
        raise ValueError("logits buffer too small for T=%d B=%d ld=%d" % (T, B, ld))
    L = _lib.lib()
    nbytes = L.slk_viterbi_kmer_workspace_bytes(T, B, nbase, klen)
    if nbytes == 0:
        raise ValueError("unsupported klen/nbase for the Viterbi kernel")
    ws = (workspace or ViterbiWorkspace()).get(nbytes, logits.device)
    scores = D.scratch(B, torch.float32, logits.device, result=True)
    paths = D.scratch((B, T), torch.int32, logits.device, result=True)
    lens = D.scratch(B, torch.int32, logits.device, result=True)
    nk = nbase ** klen
    with profiler.region("viterbi", 0.0, float(T) * B * (4.0 * S + 2.0 * nk)):
        if lengths is None:
            rc = L.slk_viterbi_kmer_logits_f32(logits.data_ptr(), ld, stats.data_ptr(), T, B, nbase, klen, float(skip_pen),
                                               float(min_prob), ws.data_ptr(), nbytes, scores.data_ptr(),
                                               paths.data_ptr(), lens.data_ptr(), D.stream_ptr())
        else:
            if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_cuda:
                raise ValueError("lengths must be an int32 device tensor with one entry per chunk")
            rc = L.slk_viterbi_kmer_logits_ragged_f32(logits.data_ptr(), ld, stats.data_ptr(), T, B, nbase, klen,
                                                      float(skip_pen), float(min_prob), lengths.data_ptr(), ws.data_ptr(),
                                                      nbytes, scores.data_ptr(), paths.data_ptr(), lens.data_ptr(),
                                                      D.stream_ptr())
    _lib.check(rc, "decode.viterbi_logits")
    return scores, paths, lens


def viterbi_fused_batch(x, pack, klen, skip_pen=0.0, nbase=4, min_prob=1e-5, workspace=None, lengths=None, lp_dump=None, plan=0):
    """basecall.decode_post(softmax layer(x)) over the batch axis from the Softmax layer's INPUT x [T, B, insize] and its
    packed weights (layers.Softmax.viterbi_pack): projection, softmax (layers.py:309-314), prepare_post (decode.py:21-36),
    log and the Viterbi forward pass (decode.py:39-82) in one kernel (csrc/softmax_viterbi.hip), then the backtrace
    (decode.py:84-91).  The logits are never written.  `lp_dump`: optional float32 device tensor [T, B, nstate] that
    receives the log-posteriors the dynamic programme consumed.  `plan`: chunks per workgroup (2, 4, or 0 = by batch size; the
    results do not depend on it).  Same outputs as viterbi_logits_batch."""
    import torch
    from . import device as D
    if klen < 3:
        raise ValueError("Kmer not long enough to apply Viterbi with skips")
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise ValueError("x must be a float32 device tensor [time, batch, features] with uniformly spaced rows")
    T, B, K = x.shape
    S = sv.nstate(klen, transducer=True, nbase=nbase)
    L = _lib.lib()
    nbytes = L.slk_softmax_viterbi_workspace_bytes(T, B, nbase, klen)      # one traceback byte per four k-mers: 256 B per (step, chunk)
    if nbytes == 0:
        raise ValueError("unsupported klen/nbase for the fused softmax + Viterbi kernel")
    ws = (workspace or ViterbiWorkspace()).get(nbytes, x.device)
    scores = D.scratch(B, torch.float32, x.device, result=True)
    paths = D.scratch((B, T), torch.int32, x.device, result=True)
    lens = D.scratch(B, torch.int32, x.device, result=True)
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_cuda):
        raise ValueError("lengths must be an int32 device tensor with one entry per chunk")
    if lp_dump is not None and (lp_dump.dtype != torch.float32 or lp_dump.numel() != T * B * S or not lp_dump.is_contiguous()):
        raise ValueError("lp_dump must be a contiguous float32 device tensor [T, B, nstate]")
    rows = float(T) * B
    # bytes: the rows of x in, one traceback byte per four k-mers out (csrc/softmax_viterbi.hip, D8) and at most the same again for the walk
    with profiler.region("softmax_viterbi", 2.0 * rows * K * S, rows * (4.0 * K + 0.5 * (nbase ** klen)),
                         f16x3_flops=2.0 * rows * K * S):
        rc = L.slk_softmax_viterbi_f32(x.data_ptr(), x.stride(1), pack.data_ptr(), K, T, B, nbase, klen, float(skip_pen),
                                       float(min_prob), lengths.data_ptr() if lengths is not None else None, int(plan), ws.data_ptr(),
                                       nbytes, scores.data_ptr(), paths.data_ptr(), lens.data_ptr(),
                                       lp_dump.data_ptr() if lp_dump is not None else None, D.stream_ptr())
    _lib.check(rc, "decode.viterbi_fused")
    return scores, paths, lens


def viterbi(post, klen, skip_pen=0.0, log=False, nbase=4):
    """Viterbi decoding of a kmer transducer (decode.py:39-93).

    :param post: A 2d array [time, nstate]
    :param klen: Length of kmer
    :param log: post array is in log space

    :returns: (score, list of k-mer states)
    """
    pd = _dev(post)
    if pd.dim() != 2:
        raise ValueError("viterbi expects a [time, state] posterior")
    scores, paths, lens = viterbi_batch(pd[:, None, :], klen, skip_pen=skip_pen, log=log, nbase=nbase)
    n = int(lens[0].item())
    return np.float32(scores[0].item()), [int(v) for v in paths[0, :n].cpu().numpy()]


def forward_max_positions():
    """The longest sequence score / forwards / forwards_batch take (slk_forward_score_max_positions: the state of a pair lives in
    the registers of one workgroup)."""
    return int(_lib.lib().slk_forward_score_max_positions())


def _forward_post(post):
    """`post` as the kernel reads it: float32 or float64, anything else is widened to float64 as numpy would (decode.py:131)."""
    import torch
    from . import device as D
    if isinstance(post, torch.Tensor):
        if post.dtype not in (torch.float32, torch.float64):
            raise ValueError("post must be float32 or float64")
        return post.to(D.device())
    a = np.asarray(post)
    if a.dtype != np.float32:
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(D.device())


def _forward_pairs(post, seqs, lengths, blank, min_prob, row_off, who, most=None):
    """The arguments of forwards_batch / forwards_backwards_batch, checked, laid out as the kernels read them and uploaded.
    most: the longest sequence `who` takes (the forward score's limit when None)."""
    import types
    import torch
    shape = tuple(post.shape)
    if len(shape) == 3 and row_off is None:
        T, B, S = shape
        packed = False
    elif len(shape) == 2 and row_off is not None:
        R, S = shape
        row_off = np.asarray(row_off, dtype=np.int64).reshape(-1)
        B = len(seqs)
        if len(row_off) not in (B, B + 1):
            raise ValueError("row_off needs one entry per pair (or one more, the end of the last)")
        if lengths is None:
            if len(row_off) != B + 1:
                raise ValueError("packed rows need lengths, or a row_off of one entry more than there are pairs")
            lengths = np.diff(row_off)
        row_off = row_off[:B]
        packed = True
    else:
        raise ValueError("%s expects a [time, batch, state] posterior, or [rows, state] with row_off" % who)
    if len(seqs) != B or B < 1:
        raise ValueError("%s needs one sequence per pair (%d sequences for %d pairs)" % (who, len(seqs), B))
    if S < 1:
        raise ValueError("posterior has no states")
    blank = int(blank)
    if blank < 0:
        blank += S
    if not 0 <= blank < S:
        raise ValueError("blank column %d outside the %d states" % (blank, S))
    seqs = [np.asarray(q).reshape(-1) for q in seqs]
    npos = [len(q) for q in seqs]
    limit = forward_max_positions() if most is None else most
    if max(npos) > limit:
        if most is not None:
            raise ValueError("a sequence of %d positions is above %s's limit of %d" % (max(npos), who, limit))
        raise ValueError("a sequence of %d positions is above the forward score's limit of %d" % (max(npos), limit))
    cat = np.concatenate(seqs).astype(np.int64) if sum(npos) else np.zeros(0, dtype=np.int64)
    if cat.size and (cat.min() < 0 or cat.max() >= S):
        raise ValueError("sequence symbols must be columns 0 .. %d of the posterior" % (S - 1))
    if min_prob is not None and not 0.0 <= float(min_prob) < 1.0:
        raise ValueError("min_prob must lie in [0, 1)")
    lens = lens_dev = None
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_cuda or packed:
            raise ValueError("device lengths must be int32 with one entry per chunk of a [time, batch, state] posterior")
        lens_dev = lengths.contiguous()
    else:
        lens = np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(-1)
        if len(lens) != B or lens.min() < 0:
            raise ValueError("lengths needs one non-negative row count per pair")
        if packed:
            if row_off.min() < 0 or (row_off + lens).max() > R:
                raise ValueError("a pair's rows lie outside the %d packed rows" % R)
        elif lens.max() > T:
            raise ValueError("a pair cannot have more than the posterior's %d rows" % T)
    if min_prob is not None and float(min_prob) > 0.0 and not str(post.dtype).endswith("float32"):
        raise ValueError("min_prob applies to float32 posteriors (decode.prepare_post is float32 arithmetic)")
    pd = _forward_post(post)
    if pd.stride(-1) != 1 or (not packed and pd.stride(0) != B * pd.stride(1)) or pd.stride(-2) < S:
        pd = pd.contiguous()
    q = types.SimpleNamespace()
    q.pd, q.ld, q.B, q.S, q.packed, q.blank, q.npos, q.lens = pd, pd.stride(-2), B, S, packed, blank, npos, lens
    q.nrows = None if packed else T
    if packed:
        q.roff, q.step = row_off, 1
    else:
        q.roff, q.step = np.arange(B, dtype=np.int64), B
    q.pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    # one upload for the offsets; the sequences and (host) lengths as int32 behind them
    q.offs = torch.as_tensor(np.concatenate([q.roff, q.pos_off])).to(pd.device)
    tail = lens.astype(np.int32) if lens_dev is None else np.zeros(1, np.int32)      # (never an empty upload)
    q.ints = torch.as_tensor(np.concatenate([cat.astype(np.int32), tail])).to(pd.device)
    q.lens_dev = lens_dev
    q.nrow_ptr = lens_dev.data_ptr() if lens_dev is not None else q.ints.data_ptr() + 4 * cat.size
    return q


def forwards_batch(post, seqs, lengths=None, full=False, blank=-1, min_prob=None, row_off=None):
    """decode.forwards (decode.py:108-139) for a batch of (posterior, sequence) pairs in one launch (csrc/forward_score.hip): the
    log-likelihood of each sequence under its posterior, summed over all alignments.

    post: float32 or float64, numpy or device tensor, either
      * [T, B, S], the network layout, read where it lies (the state axis contiguous, rows evenly spaced: a [:, :, :S] view of wider
        rows is fine); pair b runs over its first lengths[b] rows (all T when lengths is None; host integers, or an int32
        device tensor whose values the caller keeps within 0 .. T), or
      * [R, S] packed rows with row_off [B] or [B + 1] (host integers): pair b owns rows row_off[b] .. row_off[b] + lengths[b] - 1;
        lengths defaults to the differences of a [B + 1] row_off.
    seqs: one sequence of column indices per pair (a pair may have none).  blank: the column of the stay emission, -1 = the last, as
    in the reference.  min_prob: if given (float32 only), every value goes through decode.prepare_post's transform first, i.e. `post`
    is the raw network output.  full: force full length mapping.

    Returns a device float64 tensor [B].  A sequence longer than forward_max_positions() raises ValueError."""
    import torch
    from . import device as D
    q = _forward_pairs(post, seqs, lengths, blank, min_prob, row_off, "forwards_batch")
    pd, B = q.pd, q.B
    score = D.scratch(B, torch.float64, pd.device, result=True)
    L = _lib.lib()
    common = (pd.data_ptr(), q.ld, q.offs.data_ptr(), q.step, q.nrow_ptr, q.S, q.ints.data_ptr(), q.offs.data_ptr() + 8 * B, B,
              max(q.npos), q.blank, int(bool(full)))
    rows = float(sum(q.npos) + B) * (float(q.nrows) if not q.packed else float(np.mean(q.lens)))
    with profiler.region("forward_score", 3.0 * rows, rows * pd.element_size()):
        if pd.dtype == torch.float32:
            rc = L.slk_forward_score_batch_f32(*common, float(min_prob or 0.0), score.data_ptr(), D.stream_ptr())
        else:
            rc = L.slk_forward_score_batch_f64(*common, score.data_ptr(), D.stream_ptr())
    _lib.check(rc, "decode.forwards_batch")
    return score


#: most positions of a posterior row (csrc/forward_backward.hip: one 64-bit slot per column and row parity in LDS)
FORWARD_BACKWARD_MAX_STATES = 8192


def forwards_backwards_batch(post, seqs, lengths=None, full=False, blank=-1, min_prob=None, row_off=None, occupancy=True,
                             positions=True, workspace_limit=None):
    """Forward-backward over decode.forwards' recursion for a batch of (posterior, sequence) pairs (csrc/forward_backward.hip,
    design/forward_backward.md): with what probability each row emits each symbol, summed over all alignments.

    post, seqs, lengths, full, blank, min_prob, row_off: as in forwards_batch (with min_prob the occupancies refer to the transformed
    values).  At most FORWARD_BACKWARD_MAX_STATES columns.

    -> (score, occ, emit_row, emit_prob):
      score     device float64 [B], the bits forwards_batch returns;
      occ       device tensor with the shape and dtype of `post` (None unless `occupancy`): occ[t, b, c], or occ[row, c] for packed
                rows, is the probability that row t of pair b emits column c -- p[t, c] times the derivative of the score by p[t, c],
                so occ - p is the score's gradient by the logits of a softmax.  Every row of a pair with a finite score sums to 1;
                rows a pair does not own, and the rows of a `full` pair whose score is -inf, are 0;
      emit_row  list of B device int32 views (None unless `positions`): per position the row that most probably emits it (the lowest
                such row), -1 if no row can;
      emit_prob list of B device float64 views: that probability.
    The forward variables of a launch live in a workspace of 8 * 256 * ppt bytes per row of a pair (ppt = 1, 2, .. 32, the smallest
    with 256 * ppt > len(seq)); the batch runs as consecutive launches whose workspace stays within `workspace_limit` bytes (default
    transducer.WORKSPACE_LIMIT; the results do not depend on the split).  A pair that needs more on its own raises ValueError."""
    import ctypes
    import torch
    from . import device as D
    from . import transducer
    q = _forward_pairs(post, seqs, lengths, blank, min_prob, row_off, "forwards_backwards_batch")
    pd, B, S = q.pd, q.B, q.S
    if S > FORWARD_BACKWARD_MAX_STATES:
        raise ValueError("a posterior of %d states is above forward-backward's limit of %d" % (S, FORWARD_BACKWARD_MAX_STATES))
    limit = transducer.WORKSPACE_LIMIT if workspace_limit is None else int(workspace_limit)
    lens = (q.lens if q.lens is not None else q.lens_dev.cpu().numpy()).astype(np.int32)
    L = _lib.lib()

    def need(lo, hi):
        nrow = np.ascontiguousarray(lens[lo:hi])
        pos = np.ascontiguousarray(q.pos_off[lo:hi + 1])
        return int(L.slk_forward_backward_workspace_bytes(hi - lo, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p)))

    # a pair adds its rows and the 8 bytes of its offset to a launch's workspace; the table of offsets of n pairs takes less than
    # 8 n + 512 bytes (alone, a pair's takes 256)
    alone = [need(b, b + 1) for b in range(B)]
    if max(alone) > limit:
        b = int(np.argmax(alone))
        raise ValueError("pair %d needs %d bytes of workspace, above the workspace_limit of %d" % (b, alone[b], limit))
    runs = transducer.workspace_runs([n - 256 + 8 for n in alone], max(limit - 512, 0))
    dev = pd.device
    score = D.scratch(B, torch.float64, dev, result=True)
    occ = None
    if occupancy:
        # (rows no pair owns are not written by the kernel: zeros, unless every row is owned)
        whole = not q.packed and q.lens is not None and int(lens.min()) == q.nrows
        shape = tuple(pd.shape[:-1]) + (q.ld,)
        occ = (torch.empty if whole else torch.zeros)(shape, dtype=pd.dtype, device=dev)[..., :S]
    npos_all = int(q.pos_off[-1])
    erow = torch.full((max(npos_all, 1),), -1, dtype=torch.int32, device=dev) if positions else None
    eprob = torch.zeros((max(npos_all, 1),), dtype=torch.float64, device=dev) if positions else None
    ws = torch.empty(max(need(lo, hi) for lo, hi in runs), dtype=torch.uint8, device=dev)
    rows = float(sum(q.npos) + B) * (float(q.nrows) if not q.packed else float(np.mean(lens)))
    with profiler.region("forward_backward", 12.0 * rows, rows * (pd.element_size() + 16)):
        for lo, hi in runs:
            head = (pd.data_ptr(), q.ld, q.offs.data_ptr() + 8 * lo, q.step, q.nrow_ptr + 4 * lo, S, q.ints.data_ptr(),
                    q.offs.data_ptr() + 8 * (B + lo), hi - lo, max(q.npos[lo:hi]), q.blank, int(bool(full)))
            tail = (score.data_ptr() + 8 * lo, D.ptr(occ), q.ld, D.ptr(erow), D.ptr(eprob), ws.data_ptr(), need(lo, hi), D.stream_ptr())
            if pd.dtype == torch.float32:
                rc = L.slk_forward_backward_batch_f32(*head, float(min_prob or 0.0), *tail)
            else:
                rc = L.slk_forward_backward_batch_f64(*head, *tail)
            _lib.check(rc, "decode.forwards_backwards_batch")
    if positions:
        emit_row = [erow[q.pos_off[b]:q.pos_off[b + 1]] for b in range(B)]
        emit_prob = [eprob[q.pos_off[b]:q.pos_off[b + 1]] for b in range(B)]
    else:
        emit_row = emit_prob = None
    return score, occ, emit_row, emit_prob


def rescore_max_new():
    """The most new symbols one edit of rescore_edits_batch may insert (slk_rescore_edits_max_new)."""
    return int(_lib.lib().slk_rescore_edits_max_new())


class EditSet(object):
    """Candidate edits of one sequence in the layout the kernel reads: start, ndel int32 [n]; new_off int64 [n + 1]; new int32
    [new_off[-1]] -- edit i replaces positions start[i] .. start[i] + ndel[i] - 1 by new[new_off[i]:new_off[i + 1]].  Built once
    (from_list) and handed to rescore_edits_batch for every pair that carries the same sequence."""

    def __init__(self, start, ndel, new_off, new):
        self.start = np.ascontiguousarray(start, dtype=np.int32).reshape(-1)
        self.ndel = np.ascontiguousarray(ndel, dtype=np.int32).reshape(-1)
        self.new_off = np.ascontiguousarray(new_off, dtype=np.int64).reshape(-1)
        self.new = np.ascontiguousarray(new, dtype=np.int32).reshape(-1)
        if len(self.ndel) != len(self.start) or len(self.new_off) != len(self.start) + 1 or self.new_off[0] != 0 or \
                self.new_off[-1] != len(self.new) or (np.diff(self.new_off) < 0).any():
            raise ValueError("an EditSet needs one start, one ndel and one range of new symbols per edit")

    def __len__(self):
        return len(self.start)

    @classmethod
    def from_list(cls, edits):
        """From (start, ndel, new_symbols) rows."""
        news = [np.asarray(e[2], dtype=np.int64).reshape(-1) for e in edits]
        off = np.concatenate([[0], np.cumsum([len(v) for v in news])]).astype(np.int64)
        new = np.concatenate(news) if len(news) and off[-1] else np.zeros(0, dtype=np.int64)
        if new.size and (new.min() < -2 ** 31 or new.max() >= 2 ** 31):
            raise ValueError("new symbols must be columns of the posterior")
        return cls([int(e[0]) for e in edits], [int(e[1]) for e in edits], off, new)


def rescore_edits_batch(post, seqs, edits, lengths=None, blank=-1, min_prob=None, row_off=None, workspace_limit=None):
    """The full forward score of EDITED sequences (csrc/rescore_edits.hip, design/rescore_edits.md): for every pair and every
    candidate edit of its sequence, what forwards_batch(full=True) gives for the spelled-out edited sequence, up to rounding, at the
    cost of rows x (new symbols + 1) cells per candidate instead of rows x positions.

    post, seqs, lengths, blank, min_prob, row_off: as in forwards_batch; at most FORWARD_BACKWARD_MAX_STATES columns.
    edits: per pair a list of (start, ndel, new_symbols) -- replace positions start .. start + ndel - 1 of the pair's sequence by the
    columns new_symbols (none: a deletion; ndel = 0: an insertion in front of `start`) -- or an EditSet.  A pair may have none.
    ValueError for more than rescore_max_new() new symbols, an edit outside its sequence and a new symbol that is no column.

    -> (score, ll_edit): score device float64 [B], each pair's own full forward score; ll_edit a list of B device float64 views, one
    value per candidate in the caller's order (-inf when the edited sequence has more positions than the pair has rows).  A
    candidate's value depends on the pair and the candidate alone.
    The lattices of a launch live in a workspace of 16 (rows + 1) (positions + 3) bytes per pair at the most; the batch runs as
    consecutive launches whose workspace stays within `workspace_limit` bytes (default transducer.WORKSPACE_LIMIT; no bit depends
    on the split).  A pair that needs more on its own raises ValueError."""
    return _rescore_edits("rescore_edits_batch", post, seqs, edits, lengths, blank, min_prob, row_off, workspace_limit, None)


def _rescore_edits(who, post, seqs, edits, lengths, blank, min_prob, row_off, workspace_limit, band):
    """rescore_edits_batch (band None) and rescore_edits_banded_batch (band = (lo per pair, width)): one preparation of the pairs and
    the candidates, one loop over the launches; only the workspace and the entry differ."""
    import ctypes
    import types
    import torch
    from . import device as D
    from . import transducer
    q = _forward_pairs(post, seqs, lengths, blank, min_prob, row_off, who, None if band is None else BAND_MAX_POSITIONS)
    pd, B, S = q.pd, q.B, q.S
    if S > FORWARD_BACKWARD_MAX_STATES:
        raise ValueError("a posterior of %d states is above %s's limit of %d" % (S, who, FORWARD_BACKWARD_MAX_STATES))
    if len(edits) != B:
        raise ValueError("%s needs one list of edits per pair (%d for %d)" % (who, len(edits), B))
    sets = [e if isinstance(e, EditSet) else EditSet.from_list(e) for e in edits]
    L = _lib.lib()
    most = rescore_max_new()
    for b, e in enumerate(sets):
        if not len(e):
            continue
        if int(np.diff(e.new_off).max()) > most:
            raise ValueError("an edit of pair %d inserts more than %d new symbols" % (b, most))
        if e.start.min() < 0 or e.ndel.min() < 0 or int((e.start.astype(np.int64) + e.ndel).max()) > q.npos[b]:
            raise ValueError("an edit of pair %d lies outside its sequence of %d positions" % (b, q.npos[b]))
        if e.new.size and (e.new.min() < 0 or e.new.max() >= S):
            raise ValueError("new symbols must be columns 0 .. %d of the posterior" % (S - 1))
    limit = transducer.WORKSPACE_LIMIT if workspace_limit is None else int(workspace_limit)
    lens = (q.lens if q.lens is not None else q.lens_dev.cpu().numpy()).astype(np.int32)

    if band is not None:
        width = int(band[1])
        if width not in band_widths():
            raise ValueError("a band of %d states is not built: %s" % (width, ", ".join(str(w) for w in band_widths())))
        if len(band[0]) != B:
            raise ValueError("%s needs one band per pair (%d for %d)" % (who, len(band[0]), B))
        # the bands stay where they are (band_lo makes them on the device); they are checked there, one flag per pair coming back
        los = [(v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.int64))).to(pd.device).to(torch.int64).reshape(-1)
               for v in band[0]]
        for b, v in enumerate(los):
            if v.numel() != int(lens[b]) + 1:
                raise ValueError("pair %d: a band needs one entry per row index 0 .. %d, not %d" % (b, int(lens[b]), v.numel()))
        boff = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 1)]).astype(np.int64)
        cat = torch.cat(los)
        boff_dev = torch.as_tensor(boff).to(pd.device)
        first, last = boff_dev[:-1], boff_dev[1:] - 1
        falls = torch.zeros(cat.numel(), dtype=torch.int64, device=pd.device)
        falls[1:] = (cat[1:] < cat[:-1]).to(torch.int64)
        falls[first] = 0                                          # (a pair's first entry has no entry before it)
        per_pair = torch.zeros(B, dtype=torch.int64, device=pd.device).index_add_(
            0, torch.repeat_interleave(torch.arange(B, device=pd.device), last - first + 1), falls + ((cat < 0) | (cat >= 2 ** 31)))
        npos_dev = torch.as_tensor(np.asarray(q.npos, dtype=np.int64)).to(pd.device)
        bad = ((cat[first] != 0) | (per_pair > 0) | (cat[last] + width <= npos_dev)).nonzero().reshape(-1).cpu().numpy()
        if len(bad):
            b = int(bad[0])                                       # (the pair's own values say which rule it breaks)
            _check_band(los[b].cpu().numpy(), int(lens[b]), q.npos[b], width, "pair %d" % b)
            raise ValueError("pair %d: no valid band" % b)
        band_dev = cat.to(torch.int32)

    def need(lo, hi):
        nrow = np.ascontiguousarray(lens[lo:hi])
        if band is not None:
            return int(L.slk_rescore_edits_banded_workspace_bytes(hi - lo, nrow.ctypes.data_as(ctypes.c_void_p), width))
        pos = np.ascontiguousarray(q.pos_off[lo:hi + 1])
        return int(L.slk_rescore_edits_workspace_bytes(hi - lo, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p)))

    # a pair adds its lattices and 16 bytes of offsets to a launch's workspace; the offsets of n pairs take less than 16 n + 512 bytes
    # (alone, a pair's take 256)
    alone = [need(b, b + 1) for b in range(B)]
    if max(alone) > limit:
        b = int(np.argmax(alone))
        raise ValueError("pair %d needs %d bytes of workspace, above the workspace_limit of %d" % (b, alone[b], limit))
    runs = transducer.workspace_runs([n - 256 + 16 for n in alone], max(limit - 512, 0))

    # the candidates of the whole batch, sorted by (pair, start) for the launch; `order` takes them back
    count = np.array([len(e) for e in sets], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    ncand = int(coff[-1])
    dev = pd.device
    score = D.scratch(B, torch.float64, dev, result=True)
    ll = torch.empty(max(ncand, 1), dtype=torch.float64, device=dev)
    cand = None
    if ncand:
        pair = np.repeat(np.arange(B, dtype=np.int64), count)
        start = np.concatenate([e.start for e in sets]).astype(np.int64)
        ndel = np.concatenate([e.ndel for e in sets])
        nnew = np.concatenate([np.diff(e.new_off) for e in sets])
        new = np.concatenate([e.new for e in sets])
        first = np.concatenate([e.new_off[:-1] + o for e, o in zip(sets, np.concatenate([[0], np.cumsum([len(e.new) for e in sets])]))])
        order = np.argsort(pair * (int(start.max()) + 1) + start, kind="stable")
        run_lo = np.zeros(B, dtype=np.int64)
        for lo, hi in runs:
            run_lo[lo:hi] = lo
        # the sorted candidates' new symbols, gathered into their new order
        s_nnew = nnew[order]
        s_off = np.concatenate([[0], np.cumsum(s_nnew)]).astype(np.int64)
        take = np.repeat(first[order] - s_off[:-1], s_nnew) + np.arange(int(s_off[-1]), dtype=np.int64)
        ints = np.concatenate([(pair - run_lo[pair])[order], start[order], ndel[order], new[take]]).astype(np.int32)
        cand = types.SimpleNamespace(ints=torch.as_tensor(ints if ints.size else np.zeros(1, np.int32)).to(dev), off=torch.as_tensor(s_off).to(dev),
                        order=torch.as_tensor(order).to(dev))
    ws = torch.empty(max(need(lo, hi) for lo, hi in runs), dtype=torch.uint8, device=dev)
    rows = float(ncand) * (float(q.nrows) if not q.packed else float(np.mean(lens)))
    with profiler.region("rescore_edits", 20.0 * rows, 16.0 * rows):
        for lo, hi in runs:
            c0, c1 = int(coff[lo]), int(coff[hi])
            head = (pd.data_ptr(), q.ld, q.offs.data_ptr() + 8 * lo, q.step, q.nrow_ptr + 4 * lo, S, q.ints.data_ptr(),
                    q.offs.data_ptr() + 8 * (B + lo), hi - lo) + ((max(q.npos[lo:hi]),) if band is None else ()) + (q.blank,)
            if c1 > c0:
                ip = cand.ints.data_ptr()
                cands = (ip + 4 * c0, ip + 4 * (ncand + c0), ip + 4 * (2 * ncand + c0), cand.off.data_ptr() + 8 * c0, ip + 4 * 3 * ncand,
                         c1 - c0)
            else:
                cands = (None, None, None, None, None, 0)
            tail = (score.data_ptr() + 8 * lo, ll.data_ptr() + 8 * c0, ws.data_ptr(), need(lo, hi), D.stream_ptr())
            if band is not None:
                strip = (band_dev.data_ptr(), boff_dev.data_ptr() + 8 * lo, width)      # (offsets into the whole batch's lo)
                if pd.dtype == torch.float32:
                    rc = L.slk_rescore_edits_banded_batch_f32(*head, float(min_prob or 0.0), *strip, *cands, *tail)
                else:
                    rc = L.slk_rescore_edits_banded_batch_f64(*head, *strip, *cands, *tail)
            elif pd.dtype == torch.float32:
                rc = L.slk_rescore_edits_batch_f32(*head, float(min_prob or 0.0), *cands, *tail)
            else:
                rc = L.slk_rescore_edits_batch_f64(*head, *cands, *tail)
            _lib.check(rc, "decode." + who)
    if ncand:
        back = torch.empty_like(ll)
        back[cand.order] = ll                                  # (a permutation: every slot is written once)
        ll = back
    return score, [ll[coff[b]:coff[b + 1]] for b in range(B)]


#: the longest sequence the banded kernels take (csrc/rescore_band.hip: state arithmetic in int32)
BAND_MAX_POSITIONS = 2 ** 31 - 1 - 2 * 8192 - 2


def band_widths():
    """The band widths rescore_edits_banded_batch is built for: 256 states per state of a thread, up to slk_rescore_band_max_width."""
    top = int(_lib.lib().slk_rescore_band_max_width())
    return tuple(w for w in (256, 512, 1024, 2048, 4096, 8192) if w <= top)


def _check_band(lo, nrow, npos, width, what):
    """ValueError unless lo [nrow + 1] is a valid band of `width` states for `npos` positions (design/rescore_band.md 1)."""
    if len(lo) != nrow + 1:
        raise ValueError("%s: a band needs one entry per row index 0 .. %d, not %d" % (what, nrow, len(lo)))
    if lo[0] != 0 or lo.min() < 0:
        raise ValueError("%s: a band begins at state 0 and has no negative entry" % what)
    if len(lo) > 1 and (np.diff(lo) < 0).any():
        raise ValueError("%s: a band does not decrease" % what)
    if int(lo[-1]) + width <= npos:
        raise ValueError("%s: the band's last row ends at state %d, below the last of %d" % (what, int(lo[-1]) + width - 1, npos))


def band_lo(center, npos, width):
    """The band of `width` states whose rows are centred on `center` (one state per row index 0 .. T, any integer tensor or array):
    clamp(center - width // 2, 0, max(0, npos + 1 - width)), then a running maximum, on the device.  -> int32 device tensor
    [T + 1].  ValueError when that is no valid band (the centre does not begin at the sequence's start or end at its end)."""
    import torch
    from . import device as D
    c = center if isinstance(center, torch.Tensor) else torch.as_tensor(np.asarray(center, dtype=np.int64))
    c = c.to(D.device()).to(torch.int64).reshape(-1)
    if c.numel() < 1:
        raise ValueError("a band needs one centre per row index 0 .. T")
    lo = torch.cummax(torch.clamp(c - int(width) // 2, 0, max(0, int(npos) + 1 - int(width))), 0)[0].to(torch.int32)
    first, last = (int(v) for v in lo[[0, -1]].cpu())
    if first != 0 or last + int(width) <= int(npos):
        raise ValueError("a centre from %d to %d gives no band of %d states from state 0 to state %d"
                         % (int(c[0]), int(c[-1]), int(width), int(npos)))
    return lo


def band_center_from_path(path):
    """The centre of a band from a remap path (transducer.map_to_sequence*: the position each row sits at): center[0] = 0,
    center[t + 1] = path[t] + 1, the state behind row t.  -> int64 device tensor [T + 1]."""
    import torch
    from . import device as D
    p = path if isinstance(path, torch.Tensor) else torch.as_tensor(np.asarray(path, dtype=np.int64))
    p = p.to(D.device()).to(torch.int64).reshape(-1)
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=p.device), p + 1])


def band_center_from_moves(move_row, nemit, nrow, kmer_len):
    """The centre of a band over a read's own call: move_row [n] the row at which the call's path enters each of its k-mers
    (viterbi_marginals_batch), nemit [n] the letters each called k-mer emitted (the overlap rule of bio.py / csrc/bases.hip).  The
    draft's k-mer j ends with letter j + k - 1, so the k-mers passed by row t are the letters emitted in rows up to t, less k - 1,
    clipped at 0.  -> int64 device tensor [nrow + 1]."""
    import torch
    from . import device as D
    dev = D.device()
    rows = torch.as_tensor(move_row).to(dev).to(torch.int64).reshape(-1)
    emit = torch.as_tensor(nemit).to(dev).to(torch.int64).reshape(-1)
    if rows.numel() != emit.numel():
        raise ValueError("band_center_from_moves needs one letter count per move")
    per_row = torch.zeros(int(nrow) + 1, dtype=torch.int64, device=dev)
    keep = (rows >= 0) & (rows < int(nrow))
    per_row.index_add_(0, rows[keep] + 1, emit[keep])              # (row t's letters count from row index t + 1 on)
    return torch.clamp(torch.cumsum(per_row, 0) - (int(kmer_len) - 1), min=0)


def shift_center(center, edits):
    """The centre of a band after edits were applied to its sequence: every centre value above an applied edit's start moves by
    that edit's new symbols less its deleted positions.  edits: rows (start, ndel, number of new symbols) in state coordinates, or
    an EditSet.  No re-alignment: the rows keep their place.  -> int64 device tensor."""
    import torch
    from . import device as D
    c = center if isinstance(center, torch.Tensor) else torch.as_tensor(np.asarray(center, dtype=np.int64))
    c = c.to(D.device()).to(torch.int64)
    if isinstance(edits, EditSet):
        edits = list(zip(edits.start.tolist(), edits.ndel.tolist(), np.diff(edits.new_off).tolist()))
    if not len(edits):
        return c.clone()
    e = sorted((int(s), int(d), int(m)) for s, d, m in edits)
    starts = torch.as_tensor([s for s, _, _ in e], dtype=torch.int64, device=c.device)
    delta = torch.as_tensor([0] + [m - d for _, d, m in e], dtype=torch.int64, device=c.device).cumsum(0)
    return c + delta[torch.bucketize(c, starts, right=False)]     # (edits whose start lies below the value)


def rescore_edits_banded_batch(post, seqs, edits, band_lo, width, blank=-1, min_prob=None, lengths=None, row_off=None,
                               workspace_limit=None):
    """rescore_edits_batch for whole reads (csrc/rescore_band.hip, design/rescore_band.md): the lattices keep `width` states per
    row, state j in row t when band_lo[t] <= j < band_lo[t] + width, so a pair costs 16 (rows + 1) (width + 1) bytes of workspace
    whatever its sequence's length, which may be anything up to BAND_MAX_POSITIONS.

    post, seqs, edits, blank, min_prob, lengths, row_off, workspace_limit: as in rescore_edits_batch.
    band_lo: per pair one integer array or tensor [rows + 1] (decode.band_lo makes one from a centre line): it begins at 0, has no
    negative entry, does not decrease and ends with band_lo[rows] + width above the sequence's length; ValueError otherwise.
    width: one of band_widths().

    -> (score, ll_edit) as rescore_edits_batch: the log-likelihoods summed over the alignments that stay inside the band.  They
    never exceed the dense values, and have their bits when the band is all 0 and holds every state.  An edit whose columns the
    band never holds in the rows it needs scores -inf."""
    return _rescore_edits("rescore_edits_banded_batch", post, seqs, edits, lengths, blank, min_prob, row_off, workspace_limit,
                          (band_lo, width))


def rescore_edits_banded_device(post, row_off, row_step, nrow, seq, pos_off, band_lo, width, cand_off, cand_pair, cand_start, cand_ndel,
                                cand_new_off, cand_new, blank=0, min_prob=None, workspace_limit=None):
    """The launch half of rescore_edits_banded_batch, on pairs and candidates that already are device arrays in the C entry's own
    layout (design/polish_genome.md 2): nothing is listed, sorted or uploaded but the small per-pair arrays the host holds anyway.

    post: float32 or float64 device tensor whose last dimension holds the states and whose rows lie stride(-2) apart; row t of pair b
    is row row_off[b] + t * row_step of it (a [T, B, S] posterior: row_off[b] = batch index + first row * B, row_step = B).
    row_off int64 [n], nrow int32 [n]: HOST arrays (the workspace is sized from them).  seq int32 device, pos_off int64 device
    [n + 1]; band_lo int32 device, pair b's nrow[b] + 1 entries behind one another in pair order.  cand_off: HOST int64 [n + 1], the
    candidates of pair b are cand_off[b] .. cand_off[b + 1]; cand_pair (the pair, 0 .. n - 1, ascending), cand_start, cand_ndel int32
    device, cand_new_off int64 device [ncand + 1], cand_new int32 device.
    -> (score float64 device [n], ll_edit float64 device [ncand]), the bits rescore_edits_banded_batch gives the same pairs and
    candidates.  The same workspace arithmetic and the same cut into launches on pair boundaries by `workspace_limit`; cand_pair is
    rebased per launch on the device."""
    import ctypes
    import torch
    from . import device as D
    from . import transducer
    who = "rescore_edits_banded_device"
    if post.dtype not in (torch.float32, torch.float64) or not post.is_cuda or post.stride(-1) != 1:
        raise ValueError("%s takes a float32 or float64 device posterior with contiguous states" % who)
    S, ld, dev = int(post.shape[-1]), int(post.stride(-2)), post.device
    if S > FORWARD_BACKWARD_MAX_STATES:
        raise ValueError("a posterior of %d states is above %s's limit of %d" % (S, who, FORWARD_BACKWARD_MAX_STATES))
    if not 0 <= int(blank) < S:
        raise ValueError("blank column %d outside the %d states" % (blank, S))
    if int(width) not in band_widths():
        raise ValueError("a band of %d states is not built: %s" % (width, ", ".join(str(w) for w in band_widths())))
    if min_prob is not None and not 0.0 <= float(min_prob) < 1.0:
        raise ValueError("min_prob must lie in [0, 1)")
    if min_prob and post.dtype != torch.float32:
        raise ValueError("min_prob applies to float32 posteriors (decode.prepare_post is float32 arithmetic)")
    row_off = np.ascontiguousarray(row_off, dtype=np.int64).reshape(-1)
    lens = np.ascontiguousarray(nrow, dtype=np.int32).reshape(-1)
    coff = np.ascontiguousarray(cand_off, dtype=np.int64).reshape(-1)
    n = len(lens)
    if n < 1 or len(row_off) != n or len(coff) != n + 1 or pos_off.numel() != n + 1:
        raise ValueError("%s needs one row_off and nrow per pair, and one entry more of pos_off and cand_off" % who)
    rows_in_post = post.numel() // max(int(post.stride(-2)), 1) if post.is_contiguous() else None
    if lens.min() < 0 or row_off.min() < 0 or int(row_step) < 1 or \
            (rows_in_post is not None and int((row_off + np.maximum(lens.astype(np.int64) - 1, 0) * int(row_step)).max()) >= rows_in_post):
        raise ValueError("a pair's rows lie outside the posterior")
    ncand = int(coff[-1])
    if coff[0] != 0 or (np.diff(coff) < 0).any() or cand_new_off.numel() != ncand + 1 or \
            min(cand_pair.numel(), cand_start.numel(), cand_ndel.numel()) < ncand:
        raise ValueError("%s: cand_off does not describe the candidate arrays" % who)
    boff = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 1)]).astype(np.int64)
    if band_lo.dtype != torch.int32 or band_lo.numel() != int(boff[-1]):
        raise ValueError("%s needs nrow + 1 int32 band entries per pair (%d, not %d)" % (who, int(boff[-1]), band_lo.numel()))
    for name, t, dt in (("seq", seq, torch.int32), ("pos_off", pos_off, torch.int64), ("cand_pair", cand_pair, torch.int32),
                        ("cand_start", cand_start, torch.int32), ("cand_ndel", cand_ndel, torch.int32),
                        ("cand_new_off", cand_new_off, torch.int64), ("cand_new", cand_new, torch.int32)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s device tensor" % (who, name, dt))
    L = _lib.lib()
    limit = transducer.WORKSPACE_LIMIT if workspace_limit is None else int(workspace_limit)

    def need(lo, hi):
        part = np.ascontiguousarray(lens[lo:hi])
        return int(L.slk_rescore_edits_banded_workspace_bytes(hi - lo, part.ctypes.data_as(ctypes.c_void_p), int(width)))

    alone = [need(b, b + 1) for b in range(n)]
    if max(alone) > limit:
        b = int(np.argmax(alone))
        raise ValueError("pair %d needs %d bytes of workspace, above the workspace_limit of %d" % (b, alone[b], limit))
    runs = transducer.workspace_runs([v - 256 + 16 for v in alone], max(limit - 512, 0))
    roff_d, lens_d, boff_d = torch.as_tensor(row_off).to(dev), torch.as_tensor(lens).to(dev), torch.as_tensor(boff).to(dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    ll = torch.empty(max(ncand, 1), dtype=torch.float64, device=dev)
    ws = torch.empty(max(need(lo, hi) for lo, hi in runs), dtype=torch.uint8, device=dev)
    rows = float(ncand) * float(np.mean(lens))
    with profiler.region("rescore_edits", 20.0 * rows, 16.0 * rows):
        for lo, hi in runs:
            c0, c1 = int(coff[lo]), int(coff[hi])
            head = (post.data_ptr(), ld, roff_d.data_ptr() + 8 * lo, int(row_step), lens_d.data_ptr() + 4 * lo, S, seq.data_ptr(),
                    pos_off.data_ptr() + 8 * lo, hi - lo, int(blank))
            strip = (band_lo.data_ptr(), boff_d.data_ptr() + 8 * lo, int(width))
            if c1 > c0:
                local = cand_pair[c0:c1] if lo == 0 else cand_pair[c0:c1] - lo
                cands = (local.data_ptr(), cand_start.data_ptr() + 4 * c0, cand_ndel.data_ptr() + 4 * c0, cand_new_off.data_ptr() + 8 * c0,
                         cand_new.data_ptr(), c1 - c0)
            else:
                cands = (None, None, None, None, None, 0)
            tail = (score.data_ptr() + 8 * lo, ll.data_ptr() + 8 * c0, ws.data_ptr(), need(lo, hi), D.stream_ptr())
            if post.dtype == torch.float32:
                rc = L.slk_rescore_edits_banded_batch_f32(*head, float(min_prob or 0.0), *strip, *cands, *tail)
            else:
                rc = L.slk_rescore_edits_banded_batch_f64(*head, *strip, *cands, *tail)
            _lib.check(rc, "decode." + who)
    return score, ll[:ncand]


def forwards_backwards(post, seq, full=False):
    """Forward-backward for one pair with the reference's conventions (a 2-D posterior, the blank in the last column, as
    decode.forwards): -> numpy (score float64, occ [time, nstate] with the dtype of `post`, emit_row int32 [len(seq)], emit_prob
    float64 [len(seq)]); see forwards_backwards_batch."""
    if len(post.shape) != 2:
        raise ValueError("forwards_backwards expects a [time, state] posterior")
    T, S = post.shape
    score, occ, emit_row, emit_prob = forwards_backwards_batch(post, [seq], full=full, row_off=[0, T])
    return np.float64(score[0].item()), occ.cpu().numpy(), emit_row[0].cpu().numpy(), emit_prob[0].cpu().numpy()


def forwards(post, seq, full=False):
    """ The forwards score for sequence (decode.py:108-139)

    :param post: A 2D array or device tensor [time, nstate], float32 or float64; the blank is the last column
    :param seq: Sequence to map against
    :param full: Force full length mapping

    :returns: score (numpy float64)
    """
    if len(post.shape) != 2:
        raise ValueError("forwards expects a [time, state] posterior")
    T, S = post.shape
    return np.float64(forwards_batch(post, [seq], full=full, row_off=[0, T])[0].item())


def score(post, seq, full=False):
    """  Compute score of a sequence (decode.py:96-105)

    :param post: A 2D array or device tensor [time, nstate]
    :param seq: Sequence to map against
    :param full: Force full length mapping

    :returns: score
    """
    return forwards(post, seq, full=full)
