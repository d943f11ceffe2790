"""olddecode API of the reference (sloika/olddecode.py), the decoder of NON-transducer models, on the HIP kernels of
csrc/olddecode.hip.

    decode_profile(post, trans=None, log=False, slip=0.0)     olddecode.py:13-73     -> (np.float64 score, states[T])
    decode_simple(post, log=False, slip=0.0)                  olddecode.py:85-90
    estimate_transitions(post, trans=None)                    olddecode.py:93-117    -> float64 [T, 3]
    decode_post_batch(post[T,B,S], kmer_len, bad, ...)        basecall.decode_post(transducer=False), basecall.py:44, 47-50, batched
    prepare_post_drop_bad_batch / estimate_transitions_batch / decode_profile_batch: its three stages

olddecode.decode_transition (olddecode.py:76-82) is NOT mirrored: the reference cannot run it (np.copy of an itertools.repeat, then
trans[:, 1], raises IndexError).

Inputs may be numpy arrays or device tensors; posteriors are float32 (the network's dtype; float64 input is converted first).  The
dynamic programme runs in float64, as numpy runs the reference's (a float32 row plus an np.float64 weight promotes): given the same
float32 log-posteriors and float64 weights, path and score are the reference's bit for bit.  nbase is 4 (the reference asserts it,
basecall.py:48) and 3 <= kmer length <= 6.
"""
import numpy as np

from . import _lib, profiler
from .decode import ViterbiWorkspace

_ETA = 1e-10
KLEN_MIN, KLEN_MAX = 3, 6


def _dev(x):
    from . import device as D
    return D.to_dev(x)


def _check_klen(klen, nbase=4):
    if nbase != 4:
        raise ValueError("Modified bases not supported by old decoder")             # basecall.py:48
    if not KLEN_MIN <= int(klen) <= KLEN_MAX:
        raise ValueError("the profile decoder takes k-mers of length %d to %d, not %r" % (KLEN_MIN, KLEN_MAX, klen))
    return int(klen)


def klen_of(nstate):
    """k-mer length of a posterior with `nstate` k-mer columns (4^k); ValueError when there is none in range."""
    for k in range(KLEN_MIN, KLEN_MAX + 1):
        if 4 ** k == nstate:
            return k
    raise ValueError("%d states are not 4^k k-mers with %d <= k <= %d" % (nstate, KLEN_MIN, KLEN_MAX))


def _lengths_ptr(lengths, B):
    import torch
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_cuda \
            or not lengths.is_contiguous():
        raise ValueError("lengths must be a contiguous int32 device tensor with one entry per read")
    return lengths.data_ptr()


def _shape3(post, what):
    shape = tuple(post.shape)
    if len(shape) != 3:
        raise ValueError("%s expects [time, batch, state]" % what)
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError("%s: empty posterior" % what)
    return shape


def prepare_post_drop_bad_batch(post, kmer_len, min_prob=1e-5, lengths=None, nbase=4, want_rows=False):
    """decode.prepare_post(drop_bad=True) (decode.py:31-36) over the batch axis of a [T, B, 4^k + 1] posterior.
    -> device (prepared float32 [T, B, 4^k], read b left aligned in its first kept[b] rows; kept int32 [B]; with want_rows the
    indices of the rows kept, int32 [B, T], -1 padded, else None)."""
    import torch
    from . import device as D
    klen = _check_klen(kmer_len, nbase)
    T, B, S = _shape3(post, "prepare_post_drop_bad_batch")
    if S != 4 ** klen + 1:
        raise ValueError("posterior has %d states, klen=%d with a bad state needs %d" % (S, klen, 4 ** klen + 1))
    pd = _dev(post)
    lp = _lengths_ptr(lengths, B)
    out = D.scratch((T, B, S - 1), torch.float32, pd.device)
    kept = D.scratch(B, torch.int32, pd.device)
    rows = D.scratch((B, T), torch.int32, pd.device) if want_rows else None
    with profiler.region("prepare_drop_bad", 0.0, 4.0 * T * B * (2.0 * S - 1)):
        rc = _lib.lib().slk_prepare_post_drop_bad_f32(pd.data_ptr(), T, B, nbase, klen, float(min_prob), lp, out.data_ptr(),
                                                      kept.data_ptr(), D.ptr(rows), D.stream_ptr())
    _lib.check(rc, "olddecode.prepare_post_drop_bad")
    return out, kept, rows


def estimate_transitions_batch(post, trans=None, lengths=None, eta=_ETA, log=False, nbase=4):
    """olddecode.estimate_transitions over the batch axis of a prepared [T, B, 4^k] posterior -> device float64 [B, T, 3]
    (rows behind a read's length are 0); with log=True the pair (trans, log(eta + trans)) out of one pass (basecall.py:50)."""
    import torch
    from . import device as D
    if trans is not None and len(trans) != 3:
        raise ValueError("Incorrect number of transitions")                          # olddecode.py:98
    T, B, S = _shape3(post, "estimate_transitions_batch")
    klen = _check_klen(klen_of(S), nbase)
    pd = _dev(post)
    lp = _lengths_ptr(lengths, B)
    out = D.scratch((B, T, 3), torch.float64, pd.device)
    lout = D.scratch((B, T, 3), torch.float64, pd.device) if log else None
    tr = [float(v) for v in trans] if trans is not None else [0.0, 0.0, 0.0]
    with profiler.region("estimate_transitions", 30.0 * T * B * S, 8.0 * T * B * S):
        rc = _lib.lib().slk_estimate_transitions_f64(pd.data_ptr(), T, B, nbase, klen, int(trans is not None), tr[0], tr[1], tr[2],
                                                     float(eta), lp, out.data_ptr(), D.ptr(lout), D.stream_ptr())
    _lib.check(rc, "olddecode.estimate_transitions")
    return (out, lout) if log else out


def decode_profile_batch(post, trans=None, log=False, slip=0.0, lengths=None, nbase=4, workspace=None):
    """olddecode.decode_profile over the batch axis of a [T, B, 4^k] posterior (log=True: of log-posteriors).  trans: None
    (decode_simple) or a float64 device tensor [B, T, 3] of LOG weights, row t - 1 weighing the move into row t.
    -> device (scores float64 [B] (NaN for a read without rows), paths int32 [B, T] one state per row and -1 padded, lens int32 [B])."""
    import torch
    from . import device as D
    T, B, S = _shape3(post, "decode_profile_batch")
    klen = _check_klen(klen_of(S), nbase)
    if trans is not None and (not isinstance(trans, torch.Tensor) or trans.dtype != torch.float64 or tuple(trans.shape) != (B, T, 3)
                              or not trans.is_cuda or not trans.is_contiguous()):
        raise ValueError("trans must be a contiguous float64 device tensor [batch, time, 3]")
    pd = _dev(post)
    lp = _lengths_ptr(lengths, B)
    L = _lib.lib()
    nbytes = L.slk_decode_profile_workspace_bytes(T, B, nbase, klen)
    ws = (workspace or ViterbiWorkspace()).get(nbytes, pd.device)
    scores = D.scratch(B, torch.float64, pd.device, result=True)
    paths = D.scratch((B, T), torch.int32, pd.device, result=True)
    lens = D.scratch(B, torch.int32, pd.device, result=True)
    log_slip = float(np.log(_ETA + slip))                                            # olddecode.py:34
    with profiler.region("decode_profile", 0.0, float(T) * B * S * 5.0):
        rc = L.slk_decode_profile_f64(pd.data_ptr(), T, B, nbase, klen, _lib.POST_LOG if log else _lib.POST_PLAIN, D.ptr(trans),
                                      log_slip, lp, ws.data_ptr(), nbytes, scores.data_ptr(), paths.data_ptr(), lens.data_ptr(),
                                      D.stream_ptr())
    _lib.check(rc, "olddecode.decode_profile")
    return scores, paths, lens


def decode_post_batch(post, kmer_len, bad=True, min_prob=1e-5, trans=None, lengths=None, nbase=4, eta=_ETA, workspace=None):
    """basecall.decode_post(transducer=False) (basecall.py:44, 47-50) over the batch axis of a network posterior [T, B, 4^k + bad]:
    prepare_post (dropping the rows called bad and the bad column when `bad`), estimate_transitions(trans), decode_profile on
    log(eta + transitions).  lengths: int32 device tensor [B] for a ragged batch.  No host synchronisation.
    -> device (scores float64 [B], paths int32 [B, T] one state per row kept, -1 padded, lens int32 [B]; a read with no row left has
    lens 0 and score NaN)."""
    import torch
    from . import device as D
    klen = _check_klen(kmer_len, nbase)
    T, B, S = _shape3(post, "decode_post_batch")
    if S != 4 ** klen + bool(bad):
        raise ValueError("posterior does not have nstate(kmer_len) states")          # basecall.py:43
    if trans is not None and len(trans) != 3:
        raise ValueError("Incorrect number of transitions")
    if bad:
        prep, lengths, _ = prepare_post_drop_bad_batch(post, klen, min_prob, lengths, nbase)
    else:
        pd = _dev(post)
        _lengths_ptr(lengths, B)
        prep = D.scratch((T, B, S), torch.float32, pd.device)
        _lib.check(_lib.lib().slk_prepare_post_f32(pd.data_ptr(), prep.data_ptr(), pd.numel(), float(min_prob), D.stream_ptr()),
                   "decode.prepare_post")
    _, ltrans = estimate_transitions_batch(prep, trans, lengths, eta=eta, log=True, nbase=nbase)
    return decode_profile_batch(prep, ltrans, log=False, slip=0.0, lengths=lengths, nbase=nbase, workspace=workspace)


def _single(post, what):
    shape = tuple(post.shape)
    if len(shape) != 2:
        raise ValueError("%s expects a [time, state] posterior" % what)
    klen_of(shape[1])
    if shape[0] < 1:
        raise ValueError("%s: no row to decode (the reference fails with IndexError)" % what)
    return shape


def decode_profile(post, trans=None, log=False, slip=0.0):
    """Viterbi-style decoding with per-event transition weights (olddecode.py:13-73).

    :param post: posterior probabilities of kmers by event, [time, 4^k]
    :param trans: per-event log-scaled weights [stay, step, skip], one row per transition (at least time - 1 rows); None == no
        transition weights
    :param log: posterior probabilities are in log-space

    :returns: (np.float64 score, integer array with one state per event)
    """
    import torch
    T, S = _single(post, "decode_profile")
    td = None
    if trans is not None:
        tr = np.asarray(trans.cpu() if isinstance(trans, torch.Tensor) else trans, dtype=np.float64)
        if tr.ndim != 2 or tr.shape[1] != 3 or tr.shape[0] < T - 1:
            raise ValueError("trans must hold one [stay, step, skip] row per transition: at least %d rows of 3" % (T - 1))
        full = np.zeros((1, T, 3), dtype=np.float64)
        full[0, :min(T, tr.shape[0])] = tr[:T]
        td = _devf64(full)
    pd = _dev(post)
    scores, paths, lens = decode_profile_batch(pd[:, None, :], td, log=log, slip=slip)
    return np.float64(scores[0].item()), paths[0, :T].cpu().numpy().astype(np.int64)


def _devf64(x):
    import torch
    from . import device as D
    return D.to_dev(x, dtype=torch.float64)


def decode_simple(post, log=False, slip=0.0):
    """Viterbi-style decoding with uniform transitions (olddecode.py:85-90)."""
    return decode_profile(post, log=log, slip=slip)


def estimate_transitions(post, trans=None):
    """Naive estimate of transition behaviour from posteriors (olddecode.py:93-117): float64 [time, 3], rows sum to 1.

    :param post: posterior probabilities of kmers by event, [time, 4^k]
    :param trans: prior belief of transition behaviour (None = use global estimate)
    """
    from . import device as D
    if trans is not None and len(trans) != 3:
        raise ValueError("Incorrect number of transitions")
    _single(post, "estimate_transitions")
    pd = _dev(post)
    out = estimate_transitions_batch(pd[:, None, :], trans)
    return D.like_input(out[0], post)
