"""Helpers shared by the `-m gpu` parity tests (all of them call the product through its C ABI)."""
import numpy as np
import pytest


def need_gpu():
    import torch
    from sloika_amd import _lib
    if not torch.cuda.is_available() or _lib.lib().slk_device_count() < 1:
        pytest.fail("gpu-marked test needs an AMD GPU and libsloika_amd.so (no CPU fallback exists)")
    return torch


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def assert_grads_close(got, want, tol=2e-4):
    """Gradients of a training step against the float64 oracle's, relative to the largest entry of each tensor: float32 sums over
    T*B rows against float64."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, k
        scale = max(float(np.abs(w).max()), 1e-6)
        np.testing.assert_allclose(g / scale, w / scale, atol=tol, err_msg="parameter %d" % k)
