"""Event features (sloika/features.py) made on the device: csrc/event_features.hip behind slk_event_features_f32.

    from_events(ev, tag='scaled_', normalise=True, nanonet=False)      features.py:6-32

The pieces below it are what batch.chunkify / chunkify_many and pipeline.Basecaller.call_events share: the columns of one or many
event tables in ONE upload, a table of segments (whole reads or chunk windows), one launch.
"""
import numpy as np

from . import _lib


def event_columns(ev, tag='scaled_'):
    """The three columns the features are made of (features.py:18-20), in ONE dtype the kernel reads: float32 when the table
    holds nothing wider, float64 otherwise (an integer 'length' -- a count of samples -- converts exactly, and rounds to float32 once
    on the device like the reference's store into its float32 matrix).  `ev`: a numpy structured array or a dict of columns.
    -> [3, nev] array (rows mean, stdv, length)."""
    try:
        cols = [np.asarray(ev[tag + 'mean']), np.asarray(ev[tag + 'stdv']), np.asarray(ev['length'])]
    except (KeyError, ValueError, IndexError) as e:
        raise KeyError("an event table needs the columns %r, %r and 'length' (%s)" % (tag + 'mean', tag + 'stdv', e))
    if any(c.ndim != 1 or len(c) != len(cols[0]) for c in cols):
        raise ValueError("the columns of an event table are 1-D and equally long")
    if any(c.dtype.kind not in 'fiu' for c in cols):
        raise TypeError("the columns of an event table must be numeric")
    wide = any(c.dtype.kind != 'f' or c.dtype.itemsize > 4 for c in cols)
    out = np.empty((3, len(cols[0])), dtype=np.float64 if wide else np.float32)
    for k, c in enumerate(cols):
        out[k] = c
    return out


def upload_tables(tables, tag='scaled_'):
    """The columns of a list of event tables side by side in ONE device buffer (one upload): -> (device tensor [3, sum nev], off int64
    [n + 1]: table r holds events off[r] .. off[r + 1] - 1)."""
    import torch
    from . import device as D
    cols = [event_columns(ev, tag) for ev in tables]
    off = np.zeros(len(cols) + 1, dtype=np.int64)
    np.cumsum([c.shape[1] for c in cols], out=off[1:])
    wide = any(c.dtype == np.float64 for c in cols)
    host = np.empty((3, int(off[-1])), dtype=np.float64 if wide else np.float32)
    for r, c in enumerate(cols):
        host[:, off[r]:off[r + 1]] = c
    return torch.from_numpy(host).to(D.device()), off


def launch(cols, seg_start, seg_len, seg_keep, out_row, out, ld_out, normalise=True, nanonet=False):
    """One launch of slk_event_features_f32 on the current stream.  cols: [3, N] float32 / float64 device tensor (upload_tables);
    the segment table: four equally long host integer sequences (uploaded as one array); out: float32 device tensor the rows go
    into, row i of segment s at out.flatten()[4 * out_row[s] + i * ld_out:][:4].  The segments are checked against both buffers
    here, on the host: the kernel trusts them."""
    import torch
    from . import device as D
    seg = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.int64) for a in (seg_start, seg_len, seg_keep, out_row)]))
    nseg = seg.shape[1]
    if nseg == 0:
        return out
    if cols.dim() != 2 or cols.shape[0] != 3 or cols.dtype not in (torch.float32, torch.float64) or not cols.is_contiguous():
        raise ValueError("cols must be a contiguous [3, N] float32 or float64 device tensor")
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 device tensor")
    start, length, keep, row = seg
    keep = np.minimum(keep, length)
    if (start < 0).any() or (length < 0).any() or (keep < 0).any() or (row < 0).any() or (start + length > cols.shape[1]).any():
        raise ValueError("a segment lies outside the event columns")
    if (4 * row + np.maximum(keep - 1, 0) * ld_out + 4 > out.numel())[keep > 0].any():
        raise ValueError("a segment's rows lie outside the output")
    nev = cols.shape[1]
    seg_d = torch.from_numpy(seg).to(cols.device)
    rc = _lib.lib().slk_event_features_f32(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                           int(cols.dtype == torch.float64), seg_d[0].data_ptr(), seg_d[1].data_ptr(),
                                           seg_d[2].data_ptr(), nseg, int(bool(normalise)), int(bool(nanonet)), out.data_ptr(),
                                           seg_d[3].data_ptr(), int(ld_out), D.stream_ptr())
    _lib.check(rc, "event_features (%d events, %d segments)" % (nev, nseg))
    return out


def network_input(tables, nev, first=0, tag=''):
    """The features of many event tables in one upload and one launch, studentised per table, straight into the zero-padded
    [max(nev), B, 4] network input: table b's events first .. first + nev[b] - 1 become column b."""
    import torch
    from . import device as D
    cols, off = upload_tables(tables, tag)
    B = len(tables)
    x = D.scratch((max(nev), B, 4), torch.float32, cols.device).zero_()
    return launch(cols, off[:-1] + first, nev, nev, np.arange(B), x, 4 * B, normalise=True)


def from_events(ev, tag='scaled_', normalise=True, nanonet=False, device=False):
    """Create a matrix of features from an event table (features.py:6-32).

    :param ev: a numpy structured array (or a dict of columns) with fields tag + 'mean', tag + 'stdv' and 'length'
    :param tag: prefix of which fields to read
    :param normalise: perform normalisation (Studentisation) of features
    :param nanonet: use Nanonet-like features
    :param device: return the float32 device tensor instead of a numpy array

    :returns: a contiguous float32 [nev, 4] array
    """
    import torch
    cols, off = upload_tables([ev], tag)
    nev = int(off[1])
    out = torch.empty((nev, 4), dtype=torch.float32, device=cols.device)
    launch(cols, [0], [nev], [nev], [0], out, 4, normalise, nanonet)
    return out if device else out.cpu().numpy()
