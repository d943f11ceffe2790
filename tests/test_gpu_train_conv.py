"""The reverse pass of the Convolution layer (csrc/train.hip: slk_train_im2col_cin1_f32, slk_train_im2col_f32, slk_train_col2im_f32;
train.py: _conv_backward) away from the geometries tests/test_gpu_train.py trains at -- strides above one, even windows, asymmetric
padding, input samples that no window covers, rows wider than the features, more elements than one trip of the grid-stride loop --
first kernel by kernel against numpy, then the whole training step against the float64 oracle (oracle/oracle_train.py, whose gradients
of the same networks tests/test_oracle_train.py checks against finite differences)."""
import numpy as np
import pytest

from tests import conv_train_nets
from tests.gpu_util import need_gpu, dev, stream, assert_grads_close

pytestmark = pytest.mark.gpu

#: (T, B, Cin, winlen, stride, pad_lo, pad_hi)
GEOMETRIES = [
    (30, 2, 3, 4, 1, 1, 2),        # 'same', even window
    (30, 2, 3, 4, 1, 2, 1),        # 'same_left', even window
    (31, 3, 2, 5, 3, 0, 0),        # 'valid'
    (17, 2, 2, 5, 1, 4, 4),        # 'full'
    (29, 2, 6, 4, 3, 2, 1),        # the stride does not divide T + padding - winlen
    (53, 2, 3, 3, 5, 0, 0),        # stride > window: uncovered samples inside the signal
    (70, 2, 1, 16, 16, 0, 0),      # widest window and stride
    (5, 1, 12, 11, 5, 5, 5),       # shorter than the window
    (9, 3, 4, 2, 2, 0, 7),         # pad_hi larger than the window
    (40, 1, 17, 1, 1, 0, 0),       # window 1
    (23, 5, 1, 7, 2, 3, 3),        # one feature: both im2col entries
]
PAD = 3                            # columns by which the rows of the "wide" runs exceed Cin
FIRST = 1                          # ... and the column of the wider tensor at which the slice begins


def _tout(T, winlen, stride, pad_lo, pad_hi):
    return (T + pad_lo + pad_hi - winlen) // stride + 1


def _im2col_ref(x, winlen, stride, pad_lo, pad_hi):
    """include/sloika_amd.h: cols[(t*B + b)][c*winlen + k] = x(t*stride + k - pad_lo, b, c), zero outside the signal."""
    T, B, C = x.shape
    Tout = _tout(T, winlen, stride, pad_lo, pad_hi)
    src = np.arange(Tout)[:, None] * stride + np.arange(winlen)[None, :] - pad_lo          # [Tout][winlen]
    inside = (src >= 0) & (src < T)
    win = np.where(inside[:, :, None, None], x[np.clip(src, 0, T - 1)], 0)                 # [Tout][winlen][B][C]
    return np.ascontiguousarray(win.transpose(0, 2, 3, 1)).reshape(Tout * B, C * winlen).astype(x.dtype)


def _col2im_ref(dcols, T, B, C, winlen, stride, pad_lo, pad_hi):
    """The adjoint as a scatter-add in float64: tap k of window t lands on padded sample t*stride + k."""
    Tout = _tout(T, winlen, stride, pad_lo, pad_hi)
    d = np.asarray(dcols, np.float64).reshape(Tout, B, C, winlen)
    dxp = np.zeros((T + pad_lo + pad_hi, B, C))
    for k in range(winlen):
        dxp[k: k + (Tout - 1) * stride + 1: stride] += d[:, :, :, k]
    return dxp[pad_lo: pad_lo + T]


def _im2col(x, geom, wide=False):
    """slk_train_im2col_f32 on x:[T][B][Cin]; wide: x is a column slice of a tensor whose other columns hold NaN."""
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, C, w, s, lo, hi = geom
    Tout = _tout(T, w, s, lo, hi)
    assert _lib.lib().slk_conv1d_out_len(T, w, s, lo, hi) == Tout
    if wide:
        host = np.full((T, B, C + PAD), np.nan, dtype=np.float32)
        host[:, :, FIRST:FIRST + C] = x
        xd, ldx, off = dev(host), C + PAD, 4 * FIRST
    else:
        xd, ldx, off = dev(x), C, 0
    cols = torch.full((Tout * B, C * w), np.nan, dtype=torch.float32, device="cuda")
    assert _lib.lib().slk_train_im2col_f32(xd.data_ptr() + off, ldx, T, B, C, w, s, lo, hi, cols.data_ptr(), stream()) == 0
    return cols.cpu().numpy()


def _im2col_cin1(x, geom, chunk_major=False):
    """slk_train_im2col_cin1_f32 on x:[T][B][1], time-major or (as slk_conv1d_f32 takes the chunk front end's signal) chunk-major."""
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, C, w, s, lo, hi = geom
    assert C == 1
    Tout = _tout(T, w, s, lo, hi)
    if chunk_major:
        xd, xts, xbs = dev(x[:, :, 0].T), 1, T
    else:
        xd, xts, xbs = dev(x), B, 1
    cols = torch.full((Tout * B, w), np.nan, dtype=torch.float32, device="cuda")
    assert _lib.lib().slk_train_im2col_cin1_f32(xd.data_ptr(), xts, xbs, T, B, w, s, lo, hi, cols.data_ptr(), stream()) == 0
    return cols.cpu().numpy()


def _col2im(dcols, geom, wide=False):
    """slk_train_col2im_f32 into a NaN-filled dx; wide: dx is a column slice of a wider tensor, whose other columns must keep their NaN."""
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, C, w, s, lo, hi = geom
    lddx, first = (C + PAD, FIRST) if wide else (C, 0)
    dd = dev(dcols)
    dx = torch.full((T, B, lddx), np.nan, dtype=torch.float32, device="cuda")
    assert _lib.lib().slk_train_col2im_f32(dd.data_ptr(), T, B, C, w, s, lo, hi, dx.data_ptr() + 4 * first, lddx, stream()) == 0
    out = dx.cpu().numpy()
    assert np.isnan(out[:, :, :first]).all() and np.isnan(out[:, :, first + C:]).all()
    return out[:, :, first:first + C]


def _integers(rs, shape):
    return rs.randint(-8, 9, size=shape).astype(np.float32)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_im2col_is_the_gather_of_the_header(geom):
    """Both entries are gathers: equal to the numpy restatement element for element, every element of cols written (it starts as NaN),
    with rows of x wider than Cin, and -- one feature -- through both entries and both layouts of the signal."""
    T, B, C, w, s, lo, hi = geom
    x = np.random.RandomState(T + w).normal(size=(T, B, C)).astype(np.float32)
    want = _im2col_ref(x, w, s, lo, hi)
    assert np.array_equal(_im2col(x, geom), want)
    assert np.array_equal(_im2col(x, geom, wide=True), want)
    if C == 1:
        assert np.array_equal(_im2col_cin1(x, geom), want)
        assert np.array_equal(_im2col_cin1(x, geom, chunk_major=True), want)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_col2im_of_small_integers_is_exact(geom):
    """At most ceil(winlen / stride) small integers per sum: every partial sum is exact in float32, so the float64 scatter-add
    is matched to the bit -- including the zeros of the samples that no window covers (dx starts as NaN)."""
    T, B, C, w, s, lo, hi = geom
    dcols = _integers(np.random.RandomState(T + s), (_tout(T, w, s, lo, hi) * B, C * w))
    want = _col2im_ref(dcols, T, B, C, w, s, lo, hi)
    assert np.array_equal(_col2im(dcols, geom), want)
    assert np.array_equal(_col2im(dcols, geom, wide=True), want)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_col2im_of_normal_input_within_the_bound_of_a_float32_sum(geom):
    """n = ceil(winlen / stride) terms added one after the other in float32 make n - 1 rounding errors of at most 2**-24 of a partial
    sum each, to first order (n - 1) 2**-24 sum|terms|; the bound is twice that, per element (one term: exact)."""
    T, B, C, w, s, lo, hi = geom
    dcols = np.random.RandomState(T + C).normal(size=(_tout(T, w, s, lo, hi) * B, C * w)).astype(np.float32)
    want = _col2im_ref(dcols, T, B, C, w, s, lo, hi)
    bound = (-(-w // s) - 1) * 2.0 ** -23 * _col2im_ref(np.abs(dcols), T, B, C, w, s, lo, hi)
    got = _col2im(dcols, geom).astype(np.float64)
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) - bound).max())


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_col2im_is_the_adjoint_of_im2col(geom):
    """<im2col(x), c> == <x, col2im(c)> for integer-valued x and c: both sides are sums of integers, exact in float64."""
    T, B, C, w, s, lo, hi = geom
    rs = np.random.RandomState(T + B + C)
    x = _integers(rs, (T, B, C))
    c = _integers(rs, (_tout(T, w, s, lo, hi) * B, C * w))
    lhs = float(np.sum(_im2col(x, geom).astype(np.float64) * c))
    rhs = float(np.sum(x.astype(np.float64) * _col2im(c, geom)))
    assert lhs == rhs
    if C == 1:
        assert float(np.sum(_im2col_cin1(x, geom).astype(np.float64) * c)) == rhs


def test_im2col_second_trip_of_the_grid_stride_loop():
    """More outputs (18.9 M) than 65536 blocks of 256 threads: the elements past the first trip against torch's unfold view."""
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, C, w, s, lo, hi = 2048, 64, 16, 9, 1, 4, 4
    Tout = _tout(T, w, s, lo, hi)
    assert Tout * B * C * w > 65536 * 256
    x = torch.randint(-8, 9, (T, B, C), device="cuda").float()
    cols = torch.full((Tout * B, C * w), np.nan, dtype=torch.float32, device="cuda")
    assert _lib.lib().slk_train_im2col_f32(x.data_ptr(), C, T, B, C, w, s, lo, hi, cols.data_ptr(), stream()) == 0
    want = torch.nn.functional.pad(x, (0, 0, 0, 0, lo, hi)).unfold(0, w, s)             # a view [Tout][B][C][winlen]
    assert tuple(want.shape) == (Tout, B, C, w)
    assert torch.equal(cols.view(Tout, B, C, w), want)


def test_col2im_second_trip_of_the_grid_stride_loop():
    """More outputs (17.2 M) than 65536 blocks of 256 threads.  Window = stride = 2 without padding: every sample lies under exactly
    one tap, dx[2t + k][b][c] = dcols[t][b][c][k], a permuted view."""
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, C, w, s, lo, hi = 4200, 64, 64, 2, 2, 0, 0
    Tout = _tout(T, w, s, lo, hi)
    assert T * B * C > 65536 * 256 and Tout * s == T
    dcols = torch.randint(-8, 9, (Tout * B, C * w), device="cuda").float()
    dx = torch.full((T, B, C), np.nan, dtype=torch.float32, device="cuda")
    assert _lib.lib().slk_train_col2im_f32(dcols.data_ptr(), T, B, C, w, s, lo, hi, dx.data_ptr(), C, stream()) == 0
    assert torch.equal(dx.view(Tout, w, B, C), dcols.view(Tout, B, C, w).permute(0, 3, 1, 2))


def test_refusals_launch_nothing():
    """No output length, rows narrower than the features, stride 0, negative padding, null pointers: SLK_ERR_INVALID_ARG, and the
    NaN-filled outputs are as they were."""
    torch = need_gpu()
    from sloika_amd import _lib
    L, bad = _lib.lib(), _lib.SLK_ERR_INVALID_ARG
    T, B, C, w = 12, 2, 3, 5
    x = torch.zeros((T, B, C), dtype=torch.float32, device="cuda")
    cols = torch.full((T * B, C * w), np.nan, dtype=torch.float32, device="cuda")       # (room for every geometry below)
    dx = torch.full((T, B, C), np.nan, dtype=torch.float32, device="cuda")
    xp, cp, dp, st = x.data_ptr(), cols.data_ptr(), dx.data_ptr(), stream()
    # (T, Cin, ld, winlen, stride, pad_lo, pad_hi)
    for t, c, ld, win, s, lo, hi in [(3, C, C, 5, 1, 0, 0),        # Tout < 1: T = 3, winlen = 5, 'valid'
                                     (T, C, C - 1, w, 1, 2, 2),    # ldx / lddx < Cin
                                     (T, C, C, w, 0, 2, 2),        # stride 0
                                     (T, C, C, w, 1, -1, 2), (T, C, C, w, 1, 2, -1),
                                     (0, C, C, w, 1, 2, 2), (T, 0, C, w, 1, 2, 2), (T, C, C, 0, 1, 2, 2)]:
        assert L.slk_train_im2col_f32(xp, ld, t, B, c, win, s, lo, hi, cp, st) == bad
        assert L.slk_train_col2im_f32(cp, t, B, c, win, s, lo, hi, dp, ld, st) == bad
        if ld >= c > 0:
            assert L.slk_train_im2col_cin1_f32(xp, B, 1, t, B, win, s, lo, hi, cp, st) == bad
    assert L.slk_train_im2col_f32(xp, C, T, 0, C, w, 1, 2, 2, cp, st) == bad
    assert L.slk_train_col2im_f32(cp, T, 0, C, w, 1, 2, 2, dp, C, st) == bad
    assert L.slk_train_im2col_cin1_f32(xp, 0, 1, T, 0, w, 1, 2, 2, cp, st) == bad
    for a, b in ((None, cp), (xp, None)):
        assert L.slk_train_im2col_f32(a, C, T, B, C, w, 1, 2, 2, b, st) == bad
        assert L.slk_train_im2col_cin1_f32(a, B, 1, T, B, w, 1, 2, 2, b, st) == bad
    for a, b in ((None, dp), (cp, None)):
        assert L.slk_train_col2im_f32(a, T, B, C, w, 1, 2, 2, b, C, st) == bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(cols).all()) and bool(torch.isnan(dx).all())


@pytest.mark.parametrize("name", list(conv_train_nets.CASES))
def test_training_step_vs_oracle(name):
    """Loss, accuracy and every gradient of the networks of tests/conv_train_nets.py with the comparison and the figures of
    tests/test_gpu_train.py; labels as long as the network's own output (T shrinks more than once in some)."""
    need_gpu()
    from oracle import oracle_train as ot
    from sloika_amd import train
    net, spec, x, labels, weights, (min_prob, l2, drop) = conv_train_nets.make(name)
    # relu is discontinuous: no pre-activation of a relu layer so close to zero that float32 could see the other sign
    assert conv_train_nets.relu_margin(spec, ot._forward(spec, x.astype(np.float64))[1]) >= 1e-4
    want_loss, want_acc, want = ot.loss_and_grads(spec, x, labels, weights, min_prob, l2, drop)
    step = train.TrainingStep(net, min_prob=min_prob, l2=l2, drop=drop)
    loss, acc = step.forward_backward(x, labels, weights)
    assert loss == pytest.approx(want_loss, rel=2e-5)
    assert acc == pytest.approx(want_acc, abs=1e-6)
    assert_grads_close(step.gradients(), want)
