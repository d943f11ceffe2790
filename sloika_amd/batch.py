"""Chunk front end of the path (array maths of sloika/batch.py and sloika/tools/chunkify_raw.py), on the device.

    chunkify_signal(signal, chunk_len)             cut a read into [ml, chunk_len] chunks (chunkify_raw.py:172-176)
    normalise_chunks(chunks, 'per-chunk'|...)      median/MAD normalisation (chunkify_raw.py:178-185)
    chunks_to_network_input(chunks)                [ml, chunk_len] -> [chunk_len, ml, 1] (bin/train_network.py:304)
    trim_ends_and_filter, chunkify, chunkify_many  chunks of event tables with their labels (batch.py:23-87)
    remap, remap_many                              an event read mapped to its reference (batch.py:143-160)
    chunk_remap_worker, chunk_remap_many           `chunkify remap`: remap, then chunks with labels (batch.py:163-190)
    strand_list_row                                the strand-list line of a remapped read (tools/chunkify_with_remap.py:57-58)
"""
import contextlib
import os
import sys
import threading

import numpy as np

from . import _lib, profiler

DEFAULT_NORMALISATION = 'per-read'
AVAILABLE_NORMALISATIONS = frozenset(['none', 'per-read', 'per-chunk'])


def chunkify_signal(signal, chunk_len):
    """First `ml*chunk_len` samples of `signal` as [ml, chunk_len] (chunkify_raw.py:172-176)."""
    assert len(signal) >= chunk_len
    ml = len(signal) // chunk_len
    return signal[: ml * chunk_len].reshape((ml, chunk_len))


def normalise_chunks(chunks, normalisation='per-chunk', out_layout='chunk', return_stats=False):
    """(x - median) / (1.4826 * MAD), per chunk or over the whole block ('per-read'), float32, bit-identical to
    the reference's numpy evaluation.

    chunks: [ml, chunk_len] numpy or device tensor.  out_layout 'chunk' -> [ml, chunk_len];
    'network' -> [chunk_len, ml, 1] (what Layer.run consumes) written directly by the kernel.
    """
    import torch
    from . import device as D
    assert normalisation in AVAILABLE_NORMALISATIONS
    cd = D.to_dev(chunks)
    if cd.dim() != 2:
        raise ValueError("chunks must be [nchunk, chunk_len]")
    ml, chunk_len = cd.shape
    if normalisation == 'none':
        res = cd if out_layout == 'chunk' else cd.t().contiguous()[:, :, None]
        return D.like_input(res, chunks)
    L = _lib.lib()
    if normalisation == 'per-read':
        # median / MAD of the whole ml*chunk_len block (chunkify_raw.py:182-183): one "chunk" of that length
        n_units, unit_len = 1, ml * chunk_len
    else:
        n_units, unit_len = ml, chunk_len
    med = D.scratch(n_units, torch.float32, cd.device)
    mad = D.scratch(n_units, torch.float32, cd.device)
    with profiler.region("normalise", 0.0, 8.0 * ml * chunk_len):
        if out_layout == 'chunk':
            out = D.scratch((ml, chunk_len), torch.float32, cd.device)
            rc = L.slk_med_mad_normalise_f32(cd.data_ptr(), n_units, unit_len, out.data_ptr(), unit_len, 1,
                                             med.data_ptr(), mad.data_ptr(), D.stream_ptr())
        else:
            if normalisation == 'per-read':
                tmp = torch.empty((ml, chunk_len), dtype=torch.float32, device=cd.device)
                rc = L.slk_med_mad_normalise_f32(cd.data_ptr(), 1, unit_len, tmp.data_ptr(), unit_len, 1,
                                                 med.data_ptr(), mad.data_ptr(), D.stream_ptr())
                out = tmp.t().contiguous()[:, :, None]
            else:
                out = D.scratch((chunk_len, ml, 1), torch.float32, cd.device)
                rc = L.slk_med_mad_normalise_f32(cd.data_ptr(), ml, chunk_len, out.data_ptr(), 1, ml,
                                                 med.data_ptr(), mad.data_ptr(), D.stream_ptr())
    _lib.check(rc, "normalise_chunks")
    res = D.like_input(out, chunks)
    if return_stats:
        return res, D.like_input(med, chunks), D.like_input(mad, chunks)
    return res


TRIM_OPEN_PORE_LOCAL_VAR_METHODS = frozenset(['mad', 'std'])


def trim_open_pore(signal, max_op_fraction=0.3, var_method='mad', window_size=100):
    """Locate raw read in signal by thresholding local variance (sloika/batch.py:194-220).

    The per-window MADs (the array maths of the reference: `maths.mad(sig_chunks, axis=1)`) are computed on the device
    by the normalisation kernel; the percentile threshold over those few hundred numbers and the slicing are host
    logic, as in the reference.  Returns a view of `signal`.

    :param signal: raw data containing a read (1D float32, numpy or device tensor)
    :param max_op_fraction: maximum expected fraction of signal that consists of open pore
    :param var_method: 'mad' (median absolute deviation, the default) or 'std' (standard deviation) of each window
    :param window_size: size of patches used to estimate local variance
    """
    from . import device as D
    nwin = len(signal) // window_size
    sd = D.to_dev(signal)
    if sd.dim() != 1:
        raise ValueError("trim_open_pore expects a 1D signal")
    spread = _window_spread(sd[:nwin * window_size].reshape(nwin, window_size), var_method).cpu().numpy()
    # windows livelier than the max_op_fraction quantile are read; keep everything from the first to the last of them
    lively = np.flatnonzero(spread > np.percentile(spread, 100 * max_op_fraction))
    first_win, last_win = int(lively[0]), int(lively[-1])
    return signal[first_win * window_size: (last_win + 1) * window_size]


def _window_spread(windows, var_method='mad'):
    """The 'mad' or 'std' of every row of a [nwin, window_size] float32 device matrix: -> float32 device tensor [nwin]."""
    import torch
    from . import device as D
    assert var_method in TRIM_OPEN_PORE_LOCAL_VAR_METHODS, "var_method not understood: {}".format(var_method)
    if var_method == 'mad':
        return normalise_chunks(windows, 'per-chunk', return_stats=True)[2]
    windows = windows.contiguous()
    spread = torch.empty((windows.shape[0],), dtype=torch.float32, device=windows.device)
    _lib.check(_lib.lib().slk_window_std_f32(windows.data_ptr(), windows.shape[0], windows.shape[1], spread.data_ptr(),
                                             D.stream_ptr()), "window_std")
    return spread


def read_layout(lens, window_size=100):
    """The layout of a read set in one buffer: read r at off[r], padded to whole windows.  -> (strides int64 [n], off int64 [n + 1])."""
    strides = -(-np.asarray(lens, dtype=np.int64) // window_size) * window_size
    off = np.zeros(len(strides) + 1, dtype=np.int64)
    np.cumsum(strides, out=off[1:])
    return strides, off


class _Staging(threading.local):
    """Pinned host staging buffers, one per host thread and dtype, kept between calls: dtype -> (buffer, event of its last upload)."""

    def __init__(self):
        self.bufs = {}


_staging = _Staging()


@contextlib.contextmanager
def staging(total, dtype, stream=None):
    """This host thread's pinned staging buffer of `dtype`, at least `total` samples (grow-only: pinning is the expensive part), once
    the last upload out of it has left the host.  On the way out, also when the block raises, an event is recorded on `stream` (default:
    the current stream): queue every upload out of the buffer there, inside the block."""
    import torch
    buf, event = _staging.bufs.get(dtype, (None, None))
    if buf is None or buf.numel() < total:
        buf, event = torch.empty(max(total, 1 << 20), dtype=dtype).pin_memory(), None
    if event is not None:
        event.synchronize()
    try:
        yield buf
    finally:
        event = torch.cuda.Event()
        event.record(stream)
        _staging.bufs[dtype] = (buf, event)


def fill_staging(hv, signals, off, lo, hi):
    """Copy reads lo .. hi - 1 to hv[off[r]:] (hv: a staging buffer's numpy view), float32 zero-padded up to off[r + 1] (int16: the pad
    is left to slk_adc_to_pa_i16, which writes it)."""
    pad = hv.dtype == np.float32
    for r in range(lo, hi):
        end = off[r] + len(signals[r])
        hv[off[r]: end] = signals[r]
        if pad:
            hv[end: off[r + 1]] = 0.0


def _fill_set(hv, signals, off):
    """fill_staging for a whole read set, on several host threads when it is big."""
    n, total = len(signals), int(off[-1])
    if total >= (1 << 24) and n >= 16:
        # a gigabyte of samples is a tenth of a second of memcpy on one core; numpy's copies release the interpreter lock
        import concurrent.futures
        nthr = min(8, os.cpu_count() or 1)
        cuts = np.searchsorted(off, np.linspace(0, total, nthr + 1)[1:-1]).tolist()
        edges = [0] + [min(max(c, 0), n) for c in cuts] + [n]
        with concurrent.futures.ThreadPoolExecutor(nthr) as ex:
            list(ex.map(lambda k: fill_staging(hv, signals, off, edges[k], edges[k + 1]),
                        [k for k in range(nthr) if edges[k + 1] > edges[k]]))
    else:
        fill_staging(hv, signals, off, 0, n)


def upload_reads_windowed(signals, window_size=100):
    """upload_read_set for picoamperes, without the flags: -> (dev float32, off, lens)."""
    return upload_read_set(signals, window_size)[:3]


def upload_read_set(signals, window_size=100, scaling=None):
    """All reads of a set in ONE upload (through pinned memory): read r occupies `dev[off[r] : off[r] + lens[r]]`, every read padded
    with zeros to whole windows (read_layout), so that `dev.view(-1, window_size)` is the window matrix of all reads.
    -> (dev float32, off, lens, bad: bool [n], which reads hold a sample that is not finite).

    scaling: None takes `signals` as picoamperes.  Otherwise `signals` are int16 ADC reads and `scaling` their (offset, range,
    digitisation) (adc_scaling): the samples go to the device as they are (2 B each) and slk_adc_to_pa_i16 writes the picoamperes into
    the same layout -- bit for bit what the float64 reads fast5.Fast5.get_read() returns give."""
    import torch
    from . import device as D
    dtype, offset, scale = read_set_scaling(signals, scaling)
    lens = [len(s) for s in signals]
    strides, off = read_layout(lens, window_size)
    total, n = int(off[-1]), len(signals)
    with staging(total, dtype) as buf:
        _fill_set(buf.numpy(), signals, off)
        src = buf[:total].to(D.device(), non_blocking=True)
    if n == 0:
        return torch.empty((0,), dtype=torch.float32, device=src.device), off, lens, np.zeros(0, dtype=bool)
    dev, flags = picoamperes(src, _read_meta(off[:n], lens, strides, offset, scale, src.device), int(strides.max()))
    return dev, off, lens, flags.cpu().numpy() != 0


def read_set_scaling(signals, scaling):
    """How a read set crosses the bus: -> (staging dtype, per-read float64 offset and scale).  Picoamperes (scaling None) go as float32
    with offset 0 and scale 1 (nothing scales them), int16 ADC reads as they are, with adc_scaling's numbers."""
    import torch
    if scaling is None:
        return torch.float32, np.zeros(len(signals)), np.ones(len(signals))
    return (torch.int16,) + adc_scaling(signals, scaling)


def picoamperes(src, meta, max_stride):
    """An uploaded read set as float32 picoamperes, on the current stream: float32 `src` as it is, int16 ADC samples scaled into a new
    buffer (slk_adc_to_pa_i16).  meta: _read_meta's device tensors; max_stride >= every stride.  -> (set, flags int32 [n]: 1 where a
    read holds a sample that is not finite, from the same kernel)."""
    import torch
    from . import device as D
    n = int(meta[1].shape[0])
    flags = torch.zeros((n,), dtype=torch.int32, device=src.device)
    if src.dtype == torch.int16:
        return adc_to_pa(src, *meta, torch.empty(src.shape, dtype=torch.float32, device=src.device), flags, max_stride), flags
    start, lens = meta[0], meta[1]
    for lo in range(0, n, 65535):                        # the grid's y limit
        _lib.check(_lib.lib().slk_reads_nonfinite_f32(src.data_ptr(), start[lo:].data_ptr(), lens[lo:].data_ptr(), min(65535, n - lo),
                                                      max_stride, flags[lo:].data_ptr(), D.stream_ptr()), "reads_nonfinite")
    return src, flags


def adc_chunks_to_pa(adc, scaling):
    """[n, L] int16 ADC chunks (host array or device tensor) and one scaling per row (adc_scaling) -> [n, L] float32 picoamperes on the
    device, out of the active arena when there is one (Basecaller(borrow=True))."""
    import torch
    from . import device as D
    if isinstance(adc, torch.Tensor) and not adc.is_cuda:
        adc = adc.numpy()
    offset, scale = adc_scaling(adc, scaling)
    dev = D.device()
    n, length = (int(v) for v in adc.shape)
    if isinstance(adc, torch.Tensor):
        src = adc.to(dev).contiguous()
    else:
        src = D.scratch((n, length), torch.int16, dev)
        src.copy_(torch.from_numpy(np.ascontiguousarray(adc)))
    out = D.scratch((n, length), torch.float32, dev)
    if n and length:
        ln = np.full(n, length, dtype=np.int32)
        adc_to_pa(src, *_read_meta(np.arange(n, dtype=np.int64) * length, ln, ln, offset, scale, dev), out, None, length)
    return out


def adc_scaling(signals, scaling):
    """The per-read (or per-row) scaling of int16 ADC samples as the float64 arrays slk_adc_to_pa_i16 takes: -> (offset [n], scale [n]),
    scale = range / digitisation in float64, in the order of fast5.Fast5.get_read (sloika/basecall.py:105).

    signals: a list of 1-D int16 numpy arrays (reads) or one [n, L] int16 numpy array or device tensor (chunks): n rows.
    scaling: n (offset, range, digitisation) triples, an [n, 3] array in that order, or n Fast5.channel_meta dicts.
    Raises TypeError when a signal is not int16 of the right rank, ValueError when the counts or the shape of `scaling` disagree.
    Host only: nothing here touches a device."""
    try:
        import torch
        tensor = isinstance(signals, torch.Tensor)
    except ImportError:
        tensor = False
    if tensor:
        if signals.dtype != torch.int16 or signals.dim() != 2:
            raise TypeError("int16 ADC chunks must be a [n, L] int16 array, got %s %s" % (signals.dtype, tuple(signals.shape)))
        n = int(signals.shape[0])
    elif isinstance(signals, np.ndarray):
        if signals.dtype != np.int16 or signals.ndim != 2:
            raise TypeError("int16 ADC chunks must be a [n, L] int16 array, got %s %s" % (signals.dtype, signals.shape))
        n = signals.shape[0]
    else:
        for r, s in enumerate(signals):
            if not isinstance(s, np.ndarray) or s.dtype != np.int16 or s.ndim != 1:
                raise TypeError("read %d: scaling= needs 1-D int16 ADC samples, got %s" %
                                (r, "%s %s" % (s.dtype, s.shape) if isinstance(s, np.ndarray) else type(s).__name__))
        n = len(signals)
    if isinstance(scaling, np.ndarray):
        trip = np.asarray(scaling, dtype=np.float64)
        if trip.ndim != 2 or trip.shape[1] != 3:
            raise ValueError("scaling must be [n, 3] (offset, range, digitisation), got shape %s" % (scaling.shape,))
    else:
        rows = []
        for m in scaling:
            if isinstance(m, dict):
                rows.append((float(m["offset"]), float(m["range"]), float(m["digitisation"])))
            else:
                if len(m) != 3:
                    raise ValueError("a scaling triple is (offset, range, digitisation), got %r" % (m,))
                rows.append(tuple(float(v) for v in m))
        trip = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    if trip.shape[0] != n:
        raise ValueError("%d signals but %d scaling entries" % (n, trip.shape[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = trip[:, 1] / trip[:, 2]              # IEEE double division: float(range) / float(digitisation); 0 -> inf (flagged)
    return np.ascontiguousarray(trip[:, 0]), np.ascontiguousarray(scale)


def _read_meta(start, lens, strides, offset, scale, dev):
    """Per-read arrays of a read set on the device in ONE upload (through pinned memory; the device buffer comes out of the active arena
    when there is one).  -> (start int64, len int32, stride int32, offset float64, scale float64) device tensors: picoamperes' and
    slk_adc_to_pa_i16's arguments in their order."""
    import torch
    from . import device as D
    n = len(lens)
    host = torch.empty((32 * n,), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    hv[:8 * n].view(np.int64)[:] = start
    hv[8 * n:16 * n].view(np.float64)[:] = offset
    hv[16 * n:24 * n].view(np.float64)[:] = scale
    hv[24 * n:28 * n].view(np.int32)[:] = lens
    hv[28 * n:].view(np.int32)[:] = strides
    d = D.scratch((32 * n,), torch.uint8, dev)
    d.copy_(host, non_blocking=True)
    return (d[:8 * n].view(torch.int64), d[24 * n:28 * n].view(torch.int32), d[28 * n:].view(torch.int32),
            d[8 * n:16 * n].view(torch.float64), d[16 * n:24 * n].view(torch.float64))


def adc_to_pa(adc, start, lens, strides, offset, scale, out, flags, max_stride):
    """slk_adc_to_pa_i16 on device tensors: int16 `adc` -> float32 `out` (int64 start, int32 lens / strides, float64 offset / scale, flags
    int32 or None; max_stride >= every stride)."""
    from . import device as D
    with profiler.region("adc_to_pa", 0.0, 6.0 * out.numel()):
        rc = _lib.lib().slk_adc_to_pa_i16(adc.data_ptr(), start.data_ptr(), lens.data_ptr(), strides.data_ptr(), offset.data_ptr(),
                                           scale.data_ptr(), int(lens.shape[0]), int(max_stride), out.data_ptr(), D.ptr(flags),
                                           D.stream_ptr())
    _lib.check(rc, "adc_to_pa")
    return out


def open_pore_bounds_many(dev, off, lens, max_op_fraction=0.3, var_method='mad', window_size=100):
    """trim_open_pore (sloika/batch.py:194-220) for reads resident on the device as upload_read_set leaves them: the
    spreads of ALL windows in one launch, the percentile threshold per read on the host (a few hundred numbers each).
    -> list of (first sample, one past the last sample) relative to each read's start; None for a read the reference's function
    would fail on (shorter than one window, or no window livelier than the threshold)."""
    nwin = np.asarray([n // window_size for n in lens], dtype=np.int64)
    spread = _window_spread(dev.view(-1, window_size), var_method).cpu().numpy()
    w0 = np.asarray(off[:len(lens)], dtype=np.int64) // window_size
    out = [None] * len(lens)
    if max_op_fraction == 0 and len(lens):
        # np.percentile(., 0) is the minimum: all reads at once (whole windows only, as the reference's reshape leaves them)
        live = np.flatnonzero(nwin > 0)
        if len(live):
            cnt = nwin[live]
            seg0 = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            pos = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(seg0, cnt)          # window index inside its read
            vals = spread[np.repeat(w0[live], cnt) + pos]
            lively = vals > np.repeat(np.minimum.reduceat(vals, seg0), cnt)
            first = np.minimum.reduceat(np.where(lively, pos, np.iinfo(np.int64).max), seg0)
            last = np.maximum.reduceat(np.where(lively, pos, -1), seg0)
            for k, r in enumerate(live):
                if last[k] >= 0:
                    out[r] = (int(first[k]) * window_size, (int(last[k]) + 1) * window_size)
        return out
    for r, n in enumerate(nwin):
        if n < 1:
            continue
        sp = spread[w0[r]: w0[r] + n]                    # whole windows only, as the reference's reshape leaves them
        lively = np.flatnonzero(sp > np.percentile(sp, 100 * max_op_fraction))
        if len(lively):
            out[r] = (int(lively[0]) * window_size, (int(lively[-1]) + 1) * window_size)
    return out


#: why a read cannot be called, by the flag bits of slk_open_pore_trim_f32 and read_spans, in the order a read is reported by:
#: (bit, the reason on stderr (basecall.py:103-115), Basecaller.call_reads' error)
READ_FAILURES = ((1, "samples that are not finite", "read {} holds samples that are not finite"),
                 (2, "too short to trim the open pore", "read {} has no window livelier than the open-pore threshold"),
                 (4, "nothing left after trimming", "empty read after trimming (read {})"))


def read_failure(flag):
    """The READ_FAILURES row of the first bit set in `flag`; None for 0."""
    return next((row for row in READ_FAILURES if flag & row[0]), None)


def read_spans(bounds, bad, trim):
    """util.trim_array (basecall.py:111-112) on open_pore_bounds_many's bounds, as slk_open_pore_trim_f32 does it on the device:
    -> (start, lengths, flags), lists over the reads: start relative to the read's own, flags with the kernel's bits (READ_FAILURES:
    1 a sample is not finite (`bad`), 2 no whole window or no lively window, 4 nothing left after trimming).  A flagged read has
    length 0."""
    assert trim[0] >= 0 and trim[1] >= 0
    start, lengths, flags = [], [], []
    for bd, b in zip(bounds, bad):
        lo, hi, f = 0, 0, 1 if b else 0
        if bd is None:
            f |= 2
        else:
            lo, hi = bd[0] + trim[0], bd[1] - trim[1]
            f |= 4 if hi - lo < 1 else 0
        start.append(lo if f == 0 else 0)
        lengths.append(hi - lo if f == 0 else 0)
        flags.append(f)
    return start, lengths, flags


def pack_batch(dev, start, lengths, width):
    """slk_pack_reads_f32 on the current stream: the reads at dev[start[b] : start[b] + lengths[b]] -> [B, width] float32 device tensor,
    zero behind every read's end.  start / lengths: host sequences, or int64 / int32 device tensors."""
    import torch
    from . import device as D
    if not isinstance(start, torch.Tensor):
        start = torch.as_tensor(np.asarray(start, dtype=np.int64)).to(dev.device)
        lengths = torch.as_tensor(np.asarray(lengths, dtype=np.int32)).to(dev.device)
    out = torch.empty((int(lengths.shape[0]), width), dtype=torch.float32, device=dev.device)
    _lib.check(_lib.lib().slk_pack_reads_f32(dev.data_ptr(), start.data_ptr(), lengths.data_ptr(), out.shape[0], out.data_ptr(), width,
                                             D.stream_ptr()), "pack_reads")
    return out


def normalise_reads_ragged(padded, lengths):
    """Median/MAD normalisation of whole reads of different lengths over their OWN lengths (sloika/basecall.py:117-118) in one
    launch: `padded` is a [B, Lmax] float32 device tensor (read b in its first lengths[b] samples), `lengths` an int32 device
    tensor [B].  -> [Lmax, B, 1] network layout, zero behind every read's end."""
    import torch
    from . import device as D
    B, lmax = padded.shape
    out = D.scratch((lmax, B, 1), torch.float32, padded.device).zero_()
    with profiler.region("normalise", 0.0, 8.0 * B * lmax):
        rc = _lib.lib().slk_med_mad_normalise_ragged_f32(padded.data_ptr(), B, padded.stride(0), lengths.data_ptr(), out.data_ptr(),
                                                         1, B, None, None, D.stream_ptr())
    _lib.check(rc, "normalise_reads_ragged")
    return out


def chunks_to_network_input(chunks):
    """[ml, chunk_len] -> [chunk_len, ml, 1] (the transpose of bin/train_network.py:304)."""
    import torch
    if isinstance(chunks, torch.Tensor):
        return chunks.t().contiguous()[:, :, None]
    return np.ascontiguousarray(np.asarray(chunks).T)[:, :, None]


#: process-global set by init_chunk_identity_worker / init_chunk_remap_worker (sloika/batch.py:127-140)
kmer_to_state = None
kmer_alphabet = None
calc_post = None


def init_chunk_identity_worker(kmer_len, alphabet):
    """sloika/batch.py:127-129: the k-mer -> state dictionary of this process (and the alphabet it was built from, which the
    device-side label kernels take instead of a dictionary)."""
    global kmer_to_state, kmer_alphabet
    from . import bio
    kmer_to_state = bio.kmer_mapping(kmer_len, alphabet=alphabet)
    kmer_alphabet = alphabet if isinstance(alphabet, bytes) else alphabet.encode('ascii')


def init_chunk_remap_worker(model, kmer_len, alphabet):
    """sloika/batch.py:132-140: as above, plus the compiled model in the process-global `calc_post`.  `model` is a model file
    name or a Layer."""
    global calc_post
    from . import helpers, layers
    init_chunk_identity_worker(kmer_len, alphabet)
    net = model if isinstance(model, layers.Layer) else helpers.load_model(model)
    calc_post = net.compile()


# ---------------------------------------------------------------------------------------------------------------------------
# chunks of event tables (sloika/batch.py:23-87): features by csrc/event_features.hip, labels by csrc/chunk_labels.hip
# ---------------------------------------------------------------------------------------------------------------------------

def trim_ends_and_filter(ev, trim, min_length, chunk_len):
    """sloika/batch.py:23-27: `ev` without its first trim[0] and last trim[1] events, or None when it is shorter than `min_length` or
    would not fill one chunk."""
    from . import util
    if len(ev) < sum(trim) + chunk_len or len(ev) < min_length:
        return None
    return util.trim_array(ev, *trim)


def event_segments(nev, chunk_len, normalisation, first_event=0, first_row=0):
    """The segments slk_event_features_f32 takes for chunkify's features of ONE read of `nev` events (sloika/batch.py:37-60):
    -> (start, length, keep, out_row) int64 arrays, `normalise`.  'per-chunk': one segment per chunk, chunk_len + 1 events long
    where the read has one more (the delta of the chunk's last event, and that event in the chunk's moments: batch.py:43-48), chunk_len
    rows kept.  'none' / 'per-read': the whole read as one segment (moments over ALL its events), the first ml * chunk_len rows kept.
    first_event / first_row: where the read's events and its rows start in a set of reads (chunkify_many)."""
    if normalisation not in AVAILABLE_NORMALISATIONS:
        raise ValueError("normalisation must be one of %s" % sorted(AVAILABLE_NORMALISATIONS))
    if chunk_len < 1 or nev < chunk_len:
        raise ValueError("a read of %d events does not fill a chunk of %d" % (nev, chunk_len))
    ml = nev // chunk_len
    if normalisation == 'per-chunk':
        start = np.arange(ml, dtype=np.int64) * chunk_len
        length = np.minimum(start + chunk_len + 1, nev) - start
        keep = np.full(ml, chunk_len, dtype=np.int64)
        return start + first_event, length, keep, start + first_row, True
    one = np.ones(1, dtype=np.int64)
    return one * first_event, one * nev, one * (ml * chunk_len), one * first_row, normalisation == 'per-read'


def _kmer_text(ev, n):
    """The first n entries of the table's 'kmer' column as bytes: -> (contiguous 'S<k>' array, k)."""
    kmers = np.asarray(ev['kmer'][:n])
    if kmers.dtype.kind == 'U':
        kmers = kmers.astype('S')
    if kmers.dtype.kind != 'S':
        raise TypeError("the 'kmer' column must hold fixed-length strings")
    return np.ascontiguousarray(kmers), kmers.dtype.itemsize


def _chunk_features(evs, chunk_len, use_scaled, normalisation):
    """The feature half of chunkify_many (batch.py:33-62): ONE launch of slk_event_features_f32 for all reads.  -> (float32 device
    tensor [sum ml * chunk_len, 4], row_off int64 [n + 1]: read r owns rows row_off[r] .. row_off[r + 1] - 1, ml: chunks per read)."""
    import torch
    from . import features
    tag = 'scaled_' if use_scaled else ''
    nev = [len(ev['length']) for ev in evs]                    # (a structured array or a dict of columns)
    for n in nev:
        assert n >= chunk_len                                                         # batch.py:31
    ml = [n // chunk_len for n in nev]
    row_off = np.concatenate([[0], np.cumsum([m * chunk_len for m in ml])]).astype(np.int64)
    cols, off = features.upload_tables(evs, tag)
    segs = [event_segments(n, chunk_len, normalisation, int(off[r]), int(row_off[r])) for r, n in enumerate(nev)]
    feats = torch.empty((int(row_off[-1]), 4), dtype=torch.float32, device=cols.device)
    features.launch(cols, *(np.concatenate([s[k] for s in segs]) for k in range(4)), feats, 4, normalise=segs[0][4])
    return feats, row_off, ml


def chunkify_many(evs, chunk_len, kmer_len, use_scaled, normalisation, on_device=False):
    """chunkify for a list of event tables: the features of ALL reads are one launch of slk_event_features_f32, the labels one launch
    of slk_kmer_labels_i32 (compare chunkify_raw.raw_chunkify_many).  -> a list of (chunks, labels, bad) per read, each what
    chunkify gives for that read alone, bit for bit -- numpy arrays, or device tensors with on_device=True."""
    import torch
    from . import chunkify_raw, device as D
    if len(evs) == 0:
        raise ValueError("chunkify_many needs at least one event table")
    feats, row_off, ml = _chunk_features(evs, chunk_len, use_scaled, normalisation)
    total = int(row_off[-1])
    # labels: the rightmost middle k-mer's state + 1 (batch.py:69-73), 0 where the position did not change inside a chunk (:75-78)
    texts = [_kmer_text(ev, m * chunk_len) for ev, m in zip(evs, ml)]
    old_len = texts[0][1]
    if any(k != old_len for _, k in texts):
        raise ValueError("the event tables hold k-mers of different lengths")
    assert kmer_len <= old_len
    alphabet = chunkify_raw._alphabet(kmer_len)
    text = torch.from_numpy(np.frombuffer(b''.join(t.tobytes() for t, _ in texts), dtype=np.uint8).copy()).to(feats.device)
    labels = torch.empty(total, dtype=torch.int32, device=feats.device)
    status = torch.zeros(1, dtype=torch.int32, device=feats.device)
    _lib.check(_lib.lib().slk_kmer_labels_i32(text.data_ptr(), total, old_len, kmer_len, alphabet, len(alphabet), 1,
                                              labels.data_ptr(), status.data_ptr(), D.stream_ptr()), "chunkify.kmer_labels")
    seq_pos = torch.from_numpy(np.concatenate([np.asarray(ev['seq_pos'][:m * chunk_len], dtype=np.int64)
                                               for ev, m in zip(evs, ml)])).to(feats.device)
    stay = torch.zeros(total, dtype=torch.bool, device=feats.device)
    stay[1:] = seq_pos[1:] == seq_pos[:-1]
    stay[::chunk_len] = False                          # (ediff1d(..., to_begin=1): a chunk's first event always keeps its label)
    labels[stay] = 0
    chunkify_raw._status(status, "chunkify")
    out = []
    for r, ev in enumerate(evs):
        lo, hi = int(row_off[r]), int(row_off[r + 1])
        bad = np.logical_not(np.asarray(ev['good_emission'][:hi - lo])).reshape(ml[r], chunk_len)      # batch.py:80-81
        c, lab = feats[lo:hi].reshape(ml[r], chunk_len, 4), labels[lo:hi].reshape(ml[r], chunk_len)
        if on_device:
            out.append((c, lab, torch.from_numpy(bad).to(feats.device)))
        else:
            out.append((c.cpu().numpy(), lab.cpu().numpy(), bad))
    return out


def chunkify(ev, chunk_len, kmer_len, use_scaled, normalisation):
    """sloika/batch.py:30-87: the first ml * chunk_len events of the table `ev` (columns 'mean' / 'stdv' or their 'scaled_' twins,
    'length', 'kmer', 'seq_pos', 'good_emission') as training chunks: -> (chunks [ml, chunk_len, 4] float32, labels [ml, chunk_len]
    int32, bad [ml, chunk_len] bool).  The k-mer -> state mapping is the one init_chunk_identity_worker set (b'ACGT' otherwise)."""
    return chunkify_many([ev], chunk_len, kmer_len, use_scaled, normalisation)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# `chunkify remap` for event models (sloika/batch.py:143-190): the network's posterior, csrc/event_remap.hip, csrc/transducer.hip
# ---------------------------------------------------------------------------------------------------------------------------

#: the columns remap appends to the event table, in the reference's order (batch.py:157-158)
REMAP_FIELDS = ('seq_pos', 'kmer', 'good_emission')


def _remap_calc_post(calc_post_):
    f = calc_post_ if calc_post_ is not None else calc_post
    if f is None:
        raise ValueError("remap needs a compiled model: pass calc_post= or call batch.init_chunk_remap_worker first")
    return f


def _remap_network(network):
    from . import layers
    net = network if network is not None else getattr(calc_post, 'network', None)
    if not isinstance(net, layers.Layer):
        raise ValueError("remap_many needs a network: pass network= (a sloika_amd.layers.Layer) or call "
                         "batch.init_chunk_remap_worker first")
    return net


def _refuse_remap_columns(ev):
    """Raise what numpy's append_fields raises on a table that already has one of the columns remap appends (batch.py:157-158)."""
    import numpy.lib.recfunctions as nprf
    names = getattr(getattr(ev, 'dtype', None), 'names', None)
    if names is None:
        raise TypeError("remap appends columns to the event table: it must be a numpy structured array")
    if set(names) & set(REMAP_FIELDS):
        nprf.append_fields(ev[:0], list(REMAP_FIELDS), [np.zeros(0, 'i4'), np.zeros(0, 'S1'), np.zeros(0, '?')], usemask=False)
        raise ValueError("the event table already has one of the columns %s" % (REMAP_FIELDS,))


def _remapped_table(ev, path, kmers):
    import numpy.lib.recfunctions as nprf
    return nprf.append_fields(ev, list(REMAP_FIELDS), [path, kmers[path], np.repeat(True, len(ev))], usemask=False)


def _remap_priors(seqs, prior):
    from . import util
    p0 = None if prior[0] is None else [util.geometric_prior(len(q), prior[0]) for q in seqs]
    p1 = None if prior[1] is None else [util.geometric_prior(len(q), prior[1], rev=True) for q in seqs]
    return p0, p1


def remap(read_ref, ev, min_prob, kmer_len, prior, slip, calc_post=None, long_reference=False):
    """Map an event read to its reference sequence with the transducer model (sloika/batch.py:143-160):
    -> (score float32, the event table with the columns 'seq_pos' (int32), 'kmer' ('S<kmer_len>') and 'good_emission' (all True)
    appended in that order, path int32 [nev], seq = state + 1 of every k-mer of the reference).

    The features of the read (features.from_events(ev, tag=''), studentised over the read) go through `calc_post` as a
    [nev, 1, 4] batch, then decode.prepare_post and transducer.map_to_sequence(log=False), all on the device.  `prior` = (mean of
    the geometric start prior or None, the same for the end); `calc_post` defaults to the compiled model of the process
    (init_chunk_remap_worker), as in the reference.  The returned table is a plain structured array: the reference's is a numpy
    MaskedArray with nothing masked (the default of append_fields).  A table that already has one of the three columns raises what
    numpy's append_fields raises.  long_reference=True takes a reference of more than transducer.MAX_POSITIONS positions
    (transducer.map_to_sequence)."""
    from . import chunkify_raw, decode, features, transducer
    f = _remap_calc_post(calc_post)
    _refuse_remap_columns(ev)
    kmers, seq = chunkify_raw._reference_states(read_ref, kmer_len)
    inmat = features.from_events(ev, tag='', device=True)[:, None, :]
    post = decode.prepare_post(f(inmat), min_prob=min_prob, drop_bad=False)
    if post.shape[0] != len(ev):
        raise ValueError("the network gave %d steps for %d events: remap needs one step per event" % (post.shape[0], len(ev)))
    p0, p1 = _remap_priors([seq], prior)
    score, path = transducer.map_to_sequence(post, seq, slip=slip, prior_initial=None if p0 is None else p0[0],
                                             prior_final=None if p1 is None else p1[0], log=False, long_reference=long_reference)
    return score, _remapped_table(ev, path, kmers), path, seq


def _remap_many_device(refs, evs, min_prob, kmer_len, prior, slip, network, names=None, long_reference=False,
                       workspace_limit=None):
    """The launches of remap_many: -> (scores float32 device [n], paths int32 device [sum nev], ev_off host int64 [n + 1], device
    tensors of ev_off, the concatenated sequences and their offsets, [(kmers, seq)] per read)."""
    import torch
    from . import chunkify_raw, device as D, features, pipeline, transducer
    net = _remap_network(network)
    n = len(evs)
    if n == 0 or len(refs) != n:
        raise ValueError("remap_many needs one reference per read")
    names = ["read %d" % r for r in range(n)] if names is None else names
    cols = []
    for r, (ref, ev) in enumerate(zip(refs, evs)):
        _refuse_remap_columns(ev)
        npos = len(chunkify_raw._as_bytes(ref)) - kmer_len + 1
        if npos < 3:
            raise ValueError("%s cannot be remapped: its reference has %d positions, the remap needs 3" % (names[r], max(npos, 0)))
        if npos > transducer.MAX_POSITIONS and not long_reference:
            raise ValueError("%s cannot be remapped: its reference has %d positions, the remap takes %d"
                             % (names[r], npos, transducer.MAX_POSITIONS))
        c = features.event_columns(ev, '')
        if c.shape[1] < 1:
            raise ValueError("%s cannot be remapped: it has no events" % names[r])
        if not np.isfinite(c).all():
            raise ValueError("%s cannot be remapped: it holds values that are not finite" % names[r])
        cols.append(c)
    refk = [chunkify_raw._reference_states(ref, kmer_len) for ref in refs]
    seqs = [q for _, q in refk]
    nev = [c.shape[1] for c in cols]
    ev_off = np.concatenate([[0], np.cumsum(nev)]).astype(np.int64)
    # the features of all reads in one launch, straight into the zero-padded network input
    x = features.network_input([{"mean": c[0], "stdv": c[1], "length": c[2]} for c in cols], nev)
    post, steps = pipeline.Basecaller(net, kmer_len=kmer_len, min_prob=min_prob)._ragged_run(x, nev)
    if post.dim() != 3 or post.shape[1] != n or steps.cpu().numpy().tolist() != nev:
        raise ValueError("remap needs one network step per event: this network changes the number of steps")
    if post.stride(2) != 1:
        post = post.contiguous()
    nst = int(post.shape[2])
    ev_d = torch.from_numpy(ev_off).to(post.device)
    ltrans = torch.empty((int(ev_off[-1]), nst), dtype=torch.float32, device=post.device)
    with profiler.region("remap_pack", 0.0, 8.0 * ltrans.numel()):
        rc = _lib.lib().slk_remap_pack_log_post_f32(post.data_ptr(), post.stride(0), post.stride(1), int(post.shape[0]), n, nst,
                                                    steps.data_ptr(), ev_d.data_ptr(), float(min_prob), ltrans.data_ptr(),
                                                    D.stream_ptr())
    _lib.check(rc, "remap_many.pack")
    p0, p1 = _remap_priors(seqs, prior)
    limit = transducer.WORKSPACE_LIMIT if workspace_limit is None else workspace_limit
    scores, paths, ev_d, seq_d, pos_d = transducer.map_to_sequence_packed(ltrans, ev_off, seqs, slip, prior_initial=p0,
                                                                          prior_final=p1, on_device=True,
                                                                          long_reference=long_reference, workspace_limit=limit)
    return scores, paths, ev_off, ev_d, seq_d, pos_d, refk


def remap_many(refs, evs, min_prob, kmer_len, prior, slip, network=None, long_reference=False, workspace_limit=None):
    """remap (sloika/batch.py:143-160) for a list of event reads: -> a list of (score, table, path, seq), each bit for bit what remap
    gives for that read alone.  The features of all reads are one launch, the network runs once on the reads as a ragged batch
    (layers.ragged), then one slk_remap_pack_log_post_f32 and one slk_map_to_sequence_batch_f32 (one workgroup per read).
    `network`: the Layer to run; None takes the model init_chunk_remap_worker compiled.  Before anything is launched, a read that
    cannot be remapped -- fewer than 3 reference positions or more than transducer.MAX_POSITIONS, no events, a value that is not
    finite -- raises a ValueError that names it.  long_reference=True lifts the upper limit (transducer.map_to_sequence_packed: the
    remap then runs in as many launches as `workspace_limit` bytes of traceback, default transducer.WORKSPACE_LIMIT, ask for)."""
    scores, paths, ev_off, _, _, _, refk = _remap_many_device(refs, evs, min_prob, kmer_len, prior, slip, network,
                                                              long_reference=long_reference, workspace_limit=workspace_limit)
    scores, paths = scores.cpu().numpy(), paths.cpu().numpy()
    out = []
    for r, (ev, (kmers, seq)) in enumerate(zip(evs, refk)):
        path = paths[ev_off[r]:ev_off[r + 1]]
        out.append((scores[r], _remapped_table(ev, path, kmers), path, seq))
    return out


def _read_events(fn, section, segmentation):
    """(short name, events) of a worker's `fn`: a fast5 path, or an object that offers `get_section_events` and `filename_short`."""
    if hasattr(fn, 'get_section_events'):
        return fn.filename_short, fn.get_section_events(section, analysis=segmentation)
    from . import fast5
    f5 = fast5.Fast5(fn)
    return os.path.splitext(os.path.basename(fn))[0], f5.get_section_events(section, analysis=segmentation)


def chunk_remap_worker(fn, trim, min_prob, kmer_len, prior, slip, chunk_len, use_scaled, normalisation, min_length, section,
                       segmentation, references, long_reference=False):
    """Worker of `chunkify remap` for one read (sloika/batch.py:163-190): same arguments, the same tuple
    (sn + '.fast5', score, events, path, seq, chunks, labels, bad) or None with the reference's message on stderr.  `fn` is a fast5
    path read through sloika_amd.fast5.Fast5.get_section_events, or an object that offers `get_section_events(section, analysis=)`
    and `filename_short`.  The reference falls back on the stored basecall's events when the segmentation has no such section
    (get_basecall_data); that is outside this project's scope, and such a file is reported as a failure to read events.
    long_reference: as in remap."""
    try:
        sn, ev = _read_events(fn, section, segmentation)
    except Exception as e:
        sys.stderr.write('Failure reading events from {}.\n{}\n'.format(fn, repr(e)))
        return None
    try:
        read_ref = references[sn]
    except Exception as e:
        sys.stderr.write('No reference found for {}.\n{}\n'.format(fn, repr(e)))
        return None
    ev = trim_ends_and_filter(ev, trim, min_length, chunk_len)
    if ev is None:
        sys.stderr.write('{} is too short.\n'.format(fn))
        return None
    score, ev, path, seq = remap(read_ref, ev, min_prob, kmer_len, prior, slip, long_reference=long_reference)
    chunks, labels, bad_ev = chunkify(ev, chunk_len, kmer_len, use_scaled, normalisation)
    return sn + '.fast5', score, len(ev), path, seq, chunks, labels, bad_ev


def chunk_remap_many(tables, names, references, trim, min_prob, kmer_len, prior, slip, chunk_len, use_scaled, normalisation,
                     min_length, network=None, long_reference=False, workspace_limit=None):
    """chunk_remap_worker for a list of event tables in one pass: `names[r]` is the short name of read r (its key in `references`;
    messages call it by that name).  remap_many's launches first; the chunks are chunkify_many's feature launch ('scaled_' columns
    with use_scaled, the chosen normalisation); labels and the strand-list statistics come from the paths on the device
    (slk_event_remap_labels_i32), with no k-mer text in between; `bad` is all False (remap marks every emission good).
    -> (results, strand): per read the worker's tuple or None, and (nstay, start, end) or None -- strand_list_row takes both.
    A read without a reference and a read that is too short are skipped with the worker's messages; the others are unaffected.
    long_reference / workspace_limit: as in remap_many."""
    import torch
    from . import chunkify_raw, device as D
    if len(tables) != len(names):
        raise ValueError("chunk_remap_many needs one name per event table")
    results, strand = [None] * len(tables), [None] * len(tables)
    good, refs, evs = [], [], []
    for r, (ev, sn) in enumerate(zip(tables, names)):
        try:
            read_ref = references[sn]
        except Exception as e:
            sys.stderr.write('No reference found for {}.\n{}\n'.format(sn, repr(e)))
            continue
        ev = trim_ends_and_filter(ev, trim, min_length, chunk_len)
        if ev is None:
            sys.stderr.write('{} is too short.\n'.format(sn))
            continue
        good.append(r)
        refs.append(read_ref)
        evs.append(ev)
    if not good:
        return results, strand
    scores, paths, ev_off, ev_d, seq_d, pos_d, refk = _remap_many_device(refs, evs, min_prob, kmer_len, prior, slip, network,
                                                                         names=[names[r] for r in good],
                                                                         long_reference=long_reference,
                                                                         workspace_limit=workspace_limit)
    feats, row_off, ml = _chunk_features(evs, chunk_len, use_scaled, normalisation)
    total = int(row_off[-1])
    dev = feats.device
    labels = torch.empty(total, dtype=torch.int32, device=dev)
    stats = torch.empty((len(good), 3), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    row_d = torch.from_numpy(row_off).to(dev)
    _lib.check(_lib.lib().slk_event_remap_labels_i32(paths.data_ptr(), ev_d.data_ptr(), seq_d.data_ptr(), pos_d.data_ptr(), len(good),
                                                     int(chunk_len), row_d.data_ptr(), total, labels.data_ptr(), stats.data_ptr(),
                                                     status.data_ptr(), D.stream_ptr()), "chunk_remap_many.labels")
    chunkify_raw._status(status, "chunk_remap_many")
    scores, paths, feats, labels, stats = (t.cpu().numpy() for t in (scores, paths, feats, labels, stats))
    for i, r in enumerate(good):
        lo, hi = int(row_off[i]), int(row_off[i + 1])
        path = paths[ev_off[i]:ev_off[i + 1]]
        results[r] = (names[r] + '.fast5', scores[i], len(evs[i]), path, refk[i][1], feats[lo:hi].reshape(ml[i], chunk_len, 4),
                      labels[lo:hi].reshape(ml[i], chunk_len), np.zeros((ml[i], chunk_len), dtype=bool))
        strand[r] = tuple(int(v) for v in stats[i])
    return results, strand


def strand_list_row(result, stats=None):
    """The seven fields of a strand-list line (sloika/tools/chunkify_with_remap.py:57-58) for a worker's result: [filename, nev,
    -score / nev, nstay, seqlen, start, end]; the tool writes '\\t'.join(str(x) for x in them).  `stats`: the (nstay, start, end)
    chunk_remap_many returns for the read; without them they are counted from the path here."""
    read, score, nev, path, seq = result[:5]
    if stats is None:
        stats = (np.sum(np.ediff1d(path, to_begin=1) == 0), min(path), max(path))
    return [read, nev, -score / nev, stats[0], len(seq), stats[1], stats[2]]
