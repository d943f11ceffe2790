"""transducer.map_to_sequence (sloika/transducer.py:14-73) through the C ABI."""
import numpy as np

from . import _lib

_NEG_LARGE = -50000.0
_STAY = 0


def map_to_sequence(trans, sequence, slip=None, prior_initial=None, prior_final=None, log=True, long_reference=False):
    """Find Viterbi path through sequence for transducer.

    :param trans: 2D array [nev, nstate], transducer posteriors (log scaled if `log`)
    :param sequence: 1D array of state indices to be mapped against
    :param slip: slip penalty (in log-space)
    :param prior_initial / prior_final: 1D float64 arrays, prior over initial / final position
    :param long_reference: take a sequence of more than MAX_POSITIONS positions (slk_map_to_sequence_long_f32: the same score and
        path, bit for bit, with the score rows in global memory and one tile of positions in LDS); False refuses it, as the LDS-resident kernel does
    :returns: (score float32, path int32[nev])
    """
    import torch
    from . import device as D
    assert slip is None or slip >= 0.0, 'Slip penalty should be non-negative'
    if slip is None:
        # transducer.py:27 turns None into float32(nan): every slip comparison is then false and the slip
        # move always wins -- not a usable mode; refuse instead of reproducing it.
        raise ValueError("map_to_sequence needs a slip penalty (the reference's slip=None evaluates to NaN)")
    td = D.to_dev(trans)
    if td.dim() != 2:
        raise ValueError("map_to_sequence expects [time, state]")
    if not log:
        # transducer.py:30: np.log(trans)
        lt = torch.empty_like(td)
        _lib.check(_lib.lib().slk_log_post_f32(td.data_ptr(), lt.data_ptr(), td.numel(), _lib.POST_LN, 0.0, D.stream_ptr()),
                   "map_to_sequence.log")
        td = lt
    nev, nst = td.shape
    seq = torch.as_tensor(np.ascontiguousarray(sequence, dtype=np.int32)).to(td.device)
    npos = seq.shape[0]
    pi = None if prior_initial is None else torch.as_tensor(np.ascontiguousarray(prior_initial, dtype=np.float64)).to(td.device)
    pf = None if prior_final is None else torch.as_tensor(np.ascontiguousarray(prior_final, dtype=np.float64)).to(td.device)
    L = _lib.lib()
    score = torch.empty(1, dtype=torch.float32, device=td.device)
    path = torch.empty(nev, dtype=torch.int32, device=td.device)
    if long_reference and npos > MAX_POSITIONS:
        nbytes = L.slk_map_to_sequence_long_workspace_bytes(nev, npos, 0)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=td.device)
        rc = L.slk_map_to_sequence_long_f32(td.data_ptr(), nev, nst, seq.data_ptr(), npos, float(slip), D.ptr(pi), D.ptr(pf),
                                            ws.data_ptr(), nbytes, 0, score.data_ptr(), path.data_ptr(), D.stream_ptr())
    else:
        nbytes = L.slk_map_to_sequence_workspace_bytes(nev, npos)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=td.device)
        rc = L.slk_map_to_sequence_f32(td.data_ptr(), nev, nst, seq.data_ptr(), npos, float(slip), D.ptr(pi), D.ptr(pf),
                                       ws.data_ptr(), nbytes, score.data_ptr(), path.data_ptr(), D.stream_ptr())
    _lib.check(rc, "map_to_sequence")
    return np.float32(score.item()), path.cpu().numpy()


#: the tile (positions held in LDS at a time) that slk_map_to_sequence_long_f32 runs for tile = 0: MAP_LONG_TILE_DEFAULT of
#: csrc/transducer.hip (tests/test_remap_long_host.py keeps the two equal)
DEFAULT_TILE = 4096

#: the most workspace (bytes) one launch of the long-reference remap is given, unless the caller says otherwise
WORKSPACE_LIMIT = 8 << 30


def map_to_sequence_batch(trans_list, sequence_list, slip, prior_initial=None, prior_final=None, log=True, long_reference=False,
                          workspace_limit=WORKSPACE_LIMIT):
    """`map_to_sequence` for many reads in ONE launch (one workgroup per read; the reference's remap loops over reads,
    bin/chunkify.py).  `trans_list[b]`: [nev_b, nstate]; `sequence_list[b]`: state indices; priors: optional lists of
    float64 arrays (all reads or none).  long_reference / workspace_limit: see map_to_sequence_packed.
    Returns (scores float32[nread], [path int32[nev_b]])."""
    import torch
    from . import device as D
    assert slip is not None and slip >= 0.0, 'Slip penalty should be non-negative'
    nread = len(trans_list)
    if nread == 0 or len(sequence_list) != nread:
        raise ValueError("map_to_sequence_batch needs one sequence per read")
    tds = [D.to_dev(t) for t in trans_list]
    nst = tds[0].shape[1]
    if any(t.dim() != 2 or t.shape[1] != nst for t in tds):
        raise ValueError("map_to_sequence_batch expects [time, state] arrays over the same states")
    nev = [int(t.shape[0]) for t in tds]
    npos = [len(q) for q in sequence_list]
    if min(npos) < 3 or min(nev) < 1:
        raise ValueError("every read needs at least one event and three sequence positions")
    dev = tds[0].device
    td = torch.cat(tds, dim=0).contiguous()
    L = _lib.lib()
    if not log:
        lt = torch.empty_like(td)
        _lib.check(L.slk_log_post_f32(td.data_ptr(), lt.data_ptr(), td.numel(), _lib.POST_LN, 0.0, D.stream_ptr()),
                   "map_to_sequence.log")
        td = lt
    ev_off = np.concatenate([[0], np.cumsum(nev)]).astype(np.int64)
    return map_to_sequence_packed(td, ev_off, sequence_list, slip, prior_initial=prior_initial, prior_final=prior_final,
                                  long_reference=long_reference, workspace_limit=workspace_limit)


#: the longest sequence slk_map_to_sequence_batch_f32 takes: 28 bytes of LDS per position (include/sloika_amd.h); a longer one
#: needs long_reference=True (slk_map_to_sequence_long_batch_f32)
MAX_POSITIONS = 5846


def workspace_runs(nbytes, limit):
    """Cut reads with workspaces of `nbytes` each into consecutive runs [lo, hi) whose summed workspace stays within `limit`; a
    read that is above the limit on its own is a run of one."""
    runs, lo, total = [], 0, 0
    for r, n in enumerate(nbytes):
        if r > lo and total + n > limit:
            runs.append((lo, r))
            lo, total = r, 0
        total += n
    runs.append((lo, len(nbytes)))
    return runs


def map_to_sequence_packed(ltrans, ev_off, sequence_list, slip, prior_initial=None, prior_final=None, on_device=False,
                           long_reference=False, workspace_limit=WORKSPACE_LIMIT):
    """map_to_sequence_batch on what it builds first: `ltrans` is the LOG-space float32 device tensor [ev_off[-1], nstate] that holds
    the reads' rows one after the other (read b: rows ev_off[b] .. ev_off[b + 1] - 1; slk_remap_pack_log_post_f32 writes it), `ev_off`
    a host int64 array [nread + 1].  Same launch, same returns; with on_device=True the scores and the concatenated paths stay on the
    device: -> (scores float32 [nread], path int32 [ev_off[-1]], device tensors of ev_off, the sequences and their offsets).

    long_reference=True lifts the limit of MAX_POSITIONS per sequence: a call with a longer one goes to
    slk_map_to_sequence_long_batch_f32 (the same bits; a call whose reads all fit takes the entry above as before).  Its traceback
    is 4 bytes per event and position, so the reads then run as consecutive runs whose summed workspace stays within
    `workspace_limit` bytes, one launch per run (a read above the limit on its own runs alone); the results do not depend on the
    split.  workspace_limit is read only in that case."""
    import torch
    from . import device as D
    assert slip is not None and slip >= 0.0, 'Slip penalty should be non-negative'
    nread = len(sequence_list)
    ev_off = np.ascontiguousarray(ev_off, dtype=np.int64)
    if nread == 0 or len(ev_off) != nread + 1:
        raise ValueError("map_to_sequence_packed needs one sequence and one row range per read")
    if (not isinstance(ltrans, torch.Tensor) or not ltrans.is_cuda or ltrans.dtype != torch.float32 or ltrans.dim() != 2
            or not ltrans.is_contiguous() or ltrans.shape[0] != int(ev_off[-1]) or ev_off[0] != 0):
        raise ValueError("ltrans must be a contiguous float32 device tensor [ev_off[-1], nstate]")
    td, dev, nst = ltrans, ltrans.device, int(ltrans.shape[1])
    nev = np.diff(ev_off).tolist()
    npos = [len(q) for q in sequence_list]
    if min(npos) < 3 or min(nev) < 1:
        raise ValueError("every read needs at least one event and three sequence positions")
    L = _lib.lib()
    pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    use_long = bool(long_reference) and max(npos) > MAX_POSITIONS
    if use_long:
        ws_sizes = np.array([L.slk_map_to_sequence_long_workspace_bytes(e, p, 0) // 4 for e, p in zip(nev, npos)], dtype=np.int64)
    else:
        ws_sizes = np.array([e * p for e, p in zip(nev, npos)], dtype=np.int64)
    ws_off = np.concatenate([[0], np.cumsum(ws_sizes)[:-1]]).astype(np.int64)
    seq = torch.as_tensor(np.concatenate([np.asarray(q, dtype=np.int32) for q in sequence_list])).to(dev)

    def cat_prior(pl):
        if pl is None:
            return None
        if len(pl) != nread or any(len(p) != n for p, n in zip(pl, npos)):
            raise ValueError("priors must have one float64 value per sequence position of every read")
        return torch.as_tensor(np.concatenate([np.asarray(p, dtype=np.float64) for p in pl])).to(dev)
    pi, pf = cat_prior(prior_initial), cat_prior(prior_final)
    ev_d, pos_d, wso_d = (torch.as_tensor(a).to(dev) for a in (ev_off, pos_off, ws_off))
    score = torch.empty(nread, dtype=torch.float32, device=dev)
    path = torch.empty(int(ev_off[-1]), dtype=torch.int32, device=dev)
    if use_long:
        # consecutive reads are contiguous in ltrans, seq, the priors and path: a run is a pointer offset and rebased offset arrays
        runs = workspace_runs((4 * ws_sizes).tolist(), int(workspace_limit))
        ws = torch.empty(max(int(ws_sizes[lo:hi].sum()) for lo, hi in runs), dtype=torch.int32, device=dev)

        def at(t, n, size):
            return None if t is None else t.data_ptr() + int(n) * size
        for lo, hi in runs:
            e0, p0 = int(ev_off[lo]), int(pos_off[lo])
            offs = np.concatenate([ev_off[lo:hi + 1] - e0, pos_off[lo:hi + 1] - p0, ws_off[lo:hi] - ws_off[lo]])
            offs_d = torch.as_tensor(offs).to(dev)
            n1 = hi - lo + 1
            rc = L.slk_map_to_sequence_long_batch_f32(at(td, e0 * nst, 4), nst, at(offs_d, 0, 8), at(seq, p0, 4), at(offs_d, n1, 8),
                                                      hi - lo, max(npos[lo:hi]), float(slip), at(pi, p0, 8), at(pf, p0, 8),
                                                      ws.data_ptr(), at(offs_d, 2 * n1, 8), 0, at(score, lo, 4), at(path, e0, 4),
                                                      D.stream_ptr())
            _lib.check(rc, "map_to_sequence_batch")
    else:
        ws = torch.empty(int(ws_sizes.sum()), dtype=torch.int32, device=dev)
        rc = L.slk_map_to_sequence_batch_f32(td.data_ptr(), nst, ev_d.data_ptr(), seq.data_ptr(), pos_d.data_ptr(), nread,
                                             max(npos), float(slip), D.ptr(pi), D.ptr(pf), ws.data_ptr(), wso_d.data_ptr(),
                                             score.data_ptr(), path.data_ptr(), D.stream_ptr())
        _lib.check(rc, "map_to_sequence_batch")
    if on_device:
        return score, path, ev_d, seq, pos_d
    ph = path.cpu().numpy()
    return score.cpu().numpy(), [ph[ev_off[b]:ev_off[b + 1]] for b in range(nread)]
