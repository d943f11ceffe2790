"""sloika/maths.py on the device: med_mad, mad, studentise with the reference's signatures.

Numpy in, numpy out; a device tensor in, a device tensor out.  There is no host fallback: every function needs the GPU.
"""
import numpy as np


def _median(t, dim):
    """numpy's median along `dim` of a device tensor (the mean of the two middle order statistics), that dim kept."""
    import torch
    n = t.shape[dim]
    s = torch.sort(t, dim=dim).values
    lo, hi = s.narrow(dim, (n - 1) // 2, 1), s.narrow(dim, n // 2, 1)
    return (lo + hi) / 2 if t.dtype.is_floating_point else (lo + hi).to(torch.float64) / 2


def med_mad(data, factor=None, axis=None, keepdims=False):
    """Compute the Median Absolute Deviation, i.e., the median of the absolute deviations from the median, and the median
    (maths.py:4-27).

    :param data: an array (numpy or device tensor)
    :param factor: factor to scale MAD by.  Default (None) is to be consistent with the standard deviation of a normal distribution
    :param axis: for multidimensional arrays, which axis to calculate over
    :param keepdims: if True, axis is kept as dimension of length 1

    :returns: a tuple containing the median and MAD of the data

    float32 rows with the default factor -- a 1-D array, or a 2-D one along its last axis -- go through the exact selection kernels
    behind batch.normalise_chunks (bit for bit numpy's float32 evaluation); everything else is sorted on the device."""
    import torch
    from . import batch, device as D
    is_np = not isinstance(data, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(data)).to(D.device()) if is_np else data
    if t.numel() == 0:
        raise ValueError("med_mad of an empty array")
    ax = None if axis is None else int(axis) % max(t.dim(), 1)
    if factor is None and t.dtype == torch.float32 and ((t.dim() == 1 and ax in (None, 0)) or (t.dim() == 2 and ax == 1)):
        rows = t.reshape(1, -1) if t.dim() == 1 else t.contiguous()
        _, med, dmad = batch.normalise_chunks(rows, 'per-chunk', return_stats=True)
        if t.dim() == 1:
            med, dmad = (med, dmad) if (keepdims and ax is not None) else (med[0], dmad[0])
        elif keepdims:
            med, dmad = med[:, None], dmad[:, None]
    else:
        flat, dim = (t.reshape(-1), 0) if ax is None else (t, ax)
        med = _median(flat, dim)
        dmad = (1.4826 if factor is None else factor) * _median((flat - med).abs(), dim)
        if ax is None:
            med, dmad = med[0], dmad[0]
        elif not keepdims:
            med, dmad = med.squeeze(dim), dmad.squeeze(dim)
    if not is_np:
        return med, dmad
    med, dmad = med.cpu().numpy(), dmad.cpu().numpy()
    return (med[()], dmad[()]) if med.ndim == 0 else (med, dmad)


def mad(data, factor=None, axis=None, keepdims=False):
    """Compute the Median Absolute Deviation, i.e., the median of the absolute deviations from the median, and (by default) adjust
    by a factor for asymptotically normal consistency (maths.py:30-45).  Arguments as med_mad.

    :returns: the (scaled) MAD
    """
    return med_mad(data, factor=factor, axis=axis, keepdims=keepdims)[1]


def studentise(x, axis=None):
    """Studentise an array along a given axis (maths.py:48-58): (x - mean) / std, population standard deviation, a deviation that is
    not > 0 replaced by 1.

    :param x: an array (numpy or device tensor)
    :param axis: axis over which to studentise

    :returns: an array with same shape and dtype as x

    A 2-D float32 device tensor along axis 0 goes through slk_event_features_f32 (moments in float64, one rounding); everything else
    is evaluated with float64 moments by torch on the device."""
    import torch
    from . import device as D, features
    is_np = not isinstance(x, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(D.device()) if is_np else x
    if not t.dtype.is_floating_point:
        t = t.to(torch.float64)
    if not is_np and t.dim() == 2 and t.dtype == torch.float32 and axis is not None and int(axis) % 2 == 0 and t.numel() > 0:
        # three columns a launch, as the kernel's mean / stdv / length (its fourth output column is not read)
        n, ncol = t.shape
        cols = t.t().contiguous()
        out = torch.empty_like(t)
        tmp = torch.empty((n, 4), dtype=torch.float32, device=t.device)
        for c in range(0, ncol, 3):
            idx = [min(c + k, ncol - 1) for k in range(3)]
            features.launch(cols[idx].contiguous(), [0], [n], [n], [0], tmp, 4, normalise=True)
            out[:, c:c + 3] = tmp[:, :min(3, ncol - c)]
        return out
    w = t.to(torch.float64)
    dims = tuple(range(w.dim())) if axis is None else (int(axis),)
    m = w.mean(dim=dims, keepdim=True)
    s = (w - m).pow(2).mean(dim=dims, keepdim=True).sqrt()
    s = torch.where(s > 0.0, s, torch.ones_like(s))
    res = ((w - m) / s).to(t.dtype)
    return res.cpu().numpy() if is_np else res
