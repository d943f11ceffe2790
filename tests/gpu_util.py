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


# ------------------------------------------------- canaried buffers (tests/test_gpu_gru_forward_edges.py, tests/test_gpu_lstm_forward_edges.py)
GUARD = 64
PATTERN = np.uint32(0x7FC0BEEF)                # a quiet NaN with a payload nobody computes


def nan_filled(shape):
    return np.full(shape, PATTERN, np.uint32).view(np.float32)


class Out:
    """rows x width floats, rows ld apart, `lead` floats past a 16-byte boundary, PATTERN everywhere, GUARD floats on either side."""

    def __init__(self, T, B, width, ld=None, lead=0):
        self.T, self.B, self.width, self.ld, self.lead = T, B, width, ld or width, lead
        self.buf = dev(nan_filled(GUARD + lead + T * B * self.ld + GUARD))
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * (GUARD + self.lead)

    def fetch(self):
        self.host = self.buf.cpu().numpy().view(np.uint32)
        return self

    def body(self):
        a = GUARD + self.lead
        return self.host[a:a + self.T * self.B * self.ld].reshape(self.T, self.B, self.ld)

    def values(self):
        return np.ascontiguousarray(self.body()[:, :, :self.width]).view(np.float32)

    def assert_untouched_outside(self, lens, what):
        """Guards, gaps between rows, and every row at t >= lens[b]."""
        a = GUARD + self.lead
        assert (self.host[:a] == PATTERN).all() and (self.host[a + self.T * self.B * self.ld:] == PATTERN).all(), what + ": guard written"
        body = self.body()
        assert (body[:, :, self.width:] == PATTERN).all(), what + ": gap between rows written"
        if lens is not None:
            past = np.arange(self.T)[:, None] >= np.asarray(lens)[None, :]
            assert (body[past] == PATTERN).all(), what + ": row past a chunk's end written"


def padded_input(a, lens, ld):
    """[T][B][w] -> device [T][B][ld] with NaN in the gaps and in every row past a chunk's end."""
    T, B, w = a.shape
    host = nan_filled((T, B, ld))
    host[:, :, :w] = a
    if lens is not None:
        host[np.arange(T)[:, None] >= np.asarray(lens)[None, :]] = PATTERN.view(np.float32)
    return dev(host)
