"""The softmax cross-entropy head of the training step against a float64 reference of its own (tests/ref_xent.py, pinned to the
training oracle by tests/test_ref_xent.py), through the C ABI:

    A  slk_softmax_xent_grad_f32     loss terms, accuracy terms and dL/dlogits in place over given logits and row statistics
    B  slk_linear_xent_grad_f16x3    the same from the layer's input in two passes: (i) bit for bit against slk_linear_rowstats_f16x3 +
                                     slk_softmax_xent_grad_f32, (ii) against the float64 head from x, W, b directly
    C  slk_softmax_xent_eval_f32, slk_linear_xent_eval_f16x3     the validation forms
    D  underflow of a label's posterior at min_prob = 0 stays in its row (both training entries)

Cases come from tables (TABLE, IN_PLACE_ONLY, TWO_PASS_ONLY, REGIME_SHAPES), not a cross product: every value of SHAPES, NS, LDS and KS (dense rows of
x and rows K + 3 apart) occurs in the "moderate" regime at min_prob 1e-30, the four regimes x MIN_PROBS at two shapes.  In A the
kernel is handed the exact row maximum and the float64 inverse sum rounded once, so kernel and reference differ by the kernel's
arithmetic only.  Every output lies in a NaN- (int32: canary-) filled buffer with GUARD elements before and behind it; every input
is compared bit for bit with its upload afterwards.

What is asserted, per case.  Errors are in units of the row's w' = w / ((T - 2 drop) B) (1 for the validation forms):
  * gradient rows and loss rows with w' > 0: at most (BOUND[.][0] * y + BOUND[.][1]) w', y the case's largest error of the same formulas in
    plain float32 (ref_xent.head_f32) against the same float64 reference; from x (B ii, C) plus 2 w' dl, dl = 6e-7 max_j scale + 1e-6
    being the logit error tests/test_gpu_gemm.py::test_linear_rowstats_kernels_vs_float64 allows (dg_j = coef p_j (dl_j - sum_k p_k
    dl_k): a factor 2) -- and never above CAP: 2e-5 of w' for gradient elements, 2e-5 of the case's largest row loss for loss rows,
    what tests/test_gpu_validate.py (LOSS_REL) and tests/test_gpu_train.py already demand of this head;
  * flags exact: on every row on given logits; from x on the rows whose float64 top-two gap (the duplicate of a tied pair set aside)
    exceeds 2 dl, at least 90 % of the case ("flat" from x has W = 0: every logit is the bias to the last bit in any arithmetic, so
    all of its rows are exact ties of all columns and all are compared); the value on correct rows is float32(1) / float32(count);
  * exactly 0.0: rows of dropped steps, rows of zero weight, columns N .. ld-1, flag and loss rows outside the counted steps;
  * every counted row's gradient sums over its columns to within N 2^-23 w' of zero (coef (sum p - 1): no tolerance to tune).

BOUND.  Measured on an MI355X with this file (ratio = kernel error / y, both against float64; worst over the cases of a regime
whose y is at least 2^-24, so that the ratio means something; in brackets the regime's largest error, in units of w'):
                                  moderate          peaked            flat              wide
    A  gradient                   1.72 [1.9e-7]     1.26 [9.7e-8]     1.00 [1.8e-7]     1.00 [2.6e-7]
    A  loss rows                  2.52 [2.4e-6]     2.71 [8.5e-6]     2.33 [9.1e-7]     1.93 [9.1e-6]
    C  on logits, loss rows       2.92 [1.8e-6]     4.00 [7.4e-6]     1.00 [5.0e-7]     2.60 [8.5e-6]
    B  gradient                   8.02 [9.4e-7]     20.4 [2.0e-6]     1.03 [1.7e-7]     54.6 [3.8e-6]
    B  loss rows                  4.96 [2.4e-6]     6.62 [1.7e-5]     1.81 [9.4e-7]     30.4 [1.2e-5]
    C  from x, loss rows          3.19 [2.3e-6]     5.95 [1.8e-5]     0.51 [5.0e-7]     4.10 [1.6e-5]
The entries on given logits (A, C on logits) are the head's arithmetic alone: BOUND's factors are at most 4 times their worst ratio
(another seed draws other rounding errors), 1.72 for gradients and 4.00 for loss rows (a loss near 47 of which __expf's argument
scaling, |l - mx| 2^-24 relative in p, takes a few ulps).  From x the same factors hold and the product's share is the 2 w' dl term,
as derived above: B's ratios are what is left when that share is counted against the head's yardstick, not what BOUND is made of;
with the term B's and C's errors use at most 20 % of their bounds and 19 % of the caps.  BOUND[.][1] = 4 * 2^-23 of w', four float32 ulps of 1: the
gradient is coef (p - onehot) with every factor at most 1 in units of w', so a handful of roundings of a quantity near 1 is the
least any float32 evaluation can be held to; it decides where the yardstick's own draw is lucky (a case of one row) or the
coefficient vanishing (y down to 1e-18).  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest

from tests import ref_xent as rx
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = 0x5A5A1234
BOUND = {"gradient": (6.0, 4 * 2.0 ** -23), "loss": (16.0, 4 * 2.0 ** -23)}
CAP = 2e-5
SHAPES = [(1, 1, 0), (3, 1, 1), (5, 7, 0), (8, 16, 0), (16, 16, 3), (43, 3, 2), (12, 11, 5), (9, 15, 4)]        # (T, B, drop)
NS = [1, 5, 63, 64, 65, 92, 128, 129, 192, 256, 1024, 1025, 2047, 2048]
LDS = ("N", "32", "64")                                    # ld = N, N rounded up to 32, to 64
KS = [49, 64, 81, 96, 100, 112, 113, 128]
MIN_PROBS = (0.0, 1e-30, 1e-5, 1e-3, 0.5)
REGIME_SHAPES = (((12, 11, 5), 1025, 96), ((8, 16, 0), 192, 64))
UNSUPPORTED = -2


def _table():
    """(shape, N, ld mode, K, x padded): NS twice with the other axes stepping past them at different strides, then the whole 128-row
    workgroups (the branch-free epilogue, then 1 .. 4 guarded tiles behind it) that the stepping leaves out."""
    rows = []
    for i in range(2 * len(NS)):
        k, second = i % len(NS), i // len(NS)
        rows.append((SHAPES[(k + 3 * second) % len(SHAPES)], NS[k], LDS[(k + second) % 3], KS[i % len(KS)], (i // len(KS)) % 2))
    rows += [((8, 16, 0), 128, "N", 96, 0), ((16, 16, 3), 129, "64", 113, 1), ((8, 16, 0), 2048, "N", 49, 1),
             ((16, 16, 3), 1025, "32", 96, 0), ((8, 16, 0), 63, "64", 128, 1), ((16, 16, 3), 92, "N", 81, 0)]
    return rows


TABLE = _table()
#: the in-place entry alone: an ld that is no multiple of 4 (N odd, ld = N + 1) and a logits base 4 bytes past a 16-byte boundary
IN_PLACE_ONLY = [((5, 7, 0), 5, "N+1", 0), ((43, 3, 2), 65, "N+1", 0), ((12, 11, 5), 129, "N+1", 0), ((9, 15, 4), 1025, "N+1", 0),
                 ((8, 16, 0), 64, "N", 1), ((16, 16, 3), 2048, "N", 1), ((43, 3, 2), 92, "32", 1)]


#: the two-pass entry alone: pass 2 zeroing behind an odd N up to an ld that is no multiple of 4 (the guarded epilogue's scalar
#: stores), and K = 97, the first width of its seven-step instantiation
TWO_PASS_ONLY = [((5, 7, 0), 5, "N+1", 49, 1), ((43, 3, 2), 65, "N+1", 113, 0), ((16, 16, 3), 129, "N+1", 97, 0),
                 ((12, 11, 5), 1025, "N+1", 97, 1)]


def _ld(N, mode):
    return {"N": N, "N+1": N + 1, "32": (N + 31) // 32 * 32, "64": (N + 63) // 64 * 64}[mode]


def _sid(shape, N, mode):
    return "T%d-B%d-drop%d-N%d-ld%s" % (shape + (N, mode))


def _seed(shape, N, regime="moderate"):
    return 1000 * N + 7 * shape[0] + shape[1] + 100000 * rx.REGIMES.index(regime)


A_CASES = ([pytest.param(s, N, m, 0, "moderate", 1e-30, id=_sid(s, N, m) + "-moderate-mp1e-30") for s, N, m, _, _ in TABLE] +
           [pytest.param(s, N, m, sh, "moderate", 1e-30, id=_sid(s, N, m) + ("-off4" if sh else "") + "-moderate-mp1e-30")
            for s, N, m, sh in IN_PLACE_ONLY] +
           [pytest.param(s, N, "32", 0, r, mp, id=_sid(s, N, "32") + "-%s-mp%g" % (r, mp))
            for s, N, _ in REGIME_SHAPES for r in rx.REGIMES for mp in MIN_PROBS])
B_CASES = ([pytest.param(s, N, m, K, pad, "moderate", 1e-30, id=_sid(s, N, m) + "-K%d-ldx%s-moderate-mp1e-30" % (K, "K+3" if pad else "K"))
            for s, N, m, K, pad in TABLE + TWO_PASS_ONLY] +
           [pytest.param(s, N, "32", K, 0, r, mp, id=_sid(s, N, "32") + "-K%d-ldxK-%s-mp%g" % (K, r, mp))
            for s, N, K in REGIME_SHAPES for r in rx.REGIMES for mp in MIN_PROBS])
C_LOGITS = ([pytest.param(s, N, m, sh, "moderate", id=_sid(s, N, m) + ("-off4" if sh else "") + "-moderate")
             for s, N, m, sh in [t[:3] + (0,) for t in TABLE] + IN_PLACE_ONLY] +
            [pytest.param(s, N, "32", 0, r, id=_sid(s, N, "32") + "-" + r) for s, N, _ in REGIME_SHAPES for r in rx.REGIMES])
C_FROM_X = ([pytest.param(s, N, K, pad, "moderate", id="T%d-B%d-N%d-K%d-ldx%s-moderate" % (s[0], s[1], N, K, "K+3" if pad else "K"))
             for s, N, _, K, pad in TABLE] +
            [pytest.param(s, N, K, 0, r, id="T%d-B%d-N%d-K%d-ldxK-%s" % (s[0], s[1], N, K, r))
             for s, N, K in REGIME_SHAPES for r in rx.REGIMES])


# ----------------------------------------------------------------------------------------------------------- buffers
class _Out:
    """n elements on the device, NaN (float32) or CANARY (int32) everywhere, GUARD elements before and behind them; the first element
    `shift` elements past a 256-byte boundary.  `init` fills the body (the in-place logits)."""

    def __init__(self, n, dtype=np.float32, shift=0, init=None):
        self.lo, self.n = GUARD + shift, n
        self.host = np.full(self.lo + n + GUARD, np.nan if dtype == np.float32 else CANARY, dtype)
        if init is not None:
            self.host[self.lo:self.lo + n] = np.asarray(init, dtype).ravel()
        self.t = dev(self.host)
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def get(self):
        a = self.t.cpu().numpy()
        assert a[:self.lo].tobytes() == self.host[:self.lo].tobytes(), "written before the output"
        assert a[self.lo + self.n:].tobytes() == self.host[self.lo + self.n:].tobytes(), "written behind the output"
        return a[self.lo:self.lo + self.n]

    def untouched(self):
        return self.t.cpu().numpy().tobytes() == self.host.tobytes()


class _In:
    def __init__(self, a):
        self.host = np.ascontiguousarray(a)
        self.t = dev(self.host)
        self.ptr = self.t.data_ptr()

    def intact(self):
        return self.t.cpu().numpy().tobytes() == self.host.tobytes()


def _padded(a, ld):
    """Rows of a, ld apart, NaN between them."""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


class _Layer:
    """x (rows ldx apart), the weights split for the fp16 pipe, the bias: the inputs of the from-x entries."""

    def __init__(self, L, x, W, b, ldx):
        import torch
        from sloika_amd import _lib
        N, K = W.shape
        kp = (K + 15) // 16 * 16
        self.x, self.W, self.b, self.ldx, self.K, self.N = _In(_padded(x, ldx)), _In(W), _In(b), ldx, K, N
        self.hi = torch.zeros((N, kp), dtype=torch.float16, device="cuda")
        self.lo, self.inv = torch.zeros_like(self.hi), torch.zeros(N, dtype=torch.float32, device="cuda")
        _lib.check(L.slk_split_f16x2_f32(self.W.ptr, N, K, self.hi.data_ptr(), self.lo.data_ptr(), self.inv.data_ptr(), stream()), "split")
        torch.cuda.synchronize()
        self.split = [t.clone() for t in (self.hi, self.lo, self.inv)]

    def args(self):
        return (self.x.ptr, self.ldx, self.hi.data_ptr(), self.lo.data_ptr(), self.inv.data_ptr(), self.b.ptr)

    def intact(self):
        import torch
        return self.x.intact() and self.b.intact() and all(torch.equal(a, c) for a, c in zip((self.hi, self.lo, self.inv), self.split))


def _in_place(L, l, ld, shift, mx, inv, labels, weights, T, B, N, drop, min_prob):
    """slk_softmax_xent_grad_f32 on logits l (rows ld apart, NaN in columns N .. ld-1): gradient [M][ld], loss rows, flag rows."""
    import torch
    from sloika_amd import _lib
    M = T * B
    g, loss, flag = _Out(M * ld, shift=shift, init=_padded(l, ld)), _Out(M), _Out(M)
    ins = [_In(np.stack([mx, inv], axis=1).astype(np.float32)), _In(labels), _In(weights)]
    _lib.check(L.slk_softmax_xent_grad_f32(g.ptr, ld, ins[0].ptr, ins[1].ptr, ins[2].ptr, T, B, N, drop, min_prob, loss.ptr, flag.ptr,
                                           stream()), "slk_softmax_xent_grad_f32")
    torch.cuda.synchronize()
    assert all(i.intact() for i in ins), "an input changed"
    return g.get().reshape(M, ld), loss.get(), flag.get()


def _two_pass(L, lay, ld, labels, weights, T, B, drop, min_prob):
    import torch
    from sloika_amd import _lib
    M = T * B
    g, loss, flag, xrow = _Out(M * ld), _Out(M), _Out(M), _Out(4 * M)
    ins = [_In(labels), _In(weights)]
    _lib.check(L.slk_linear_xent_grad_f16x3(*lay.args(), g.ptr, ld, lay.K, lay.N, ins[0].ptr, ins[1].ptr, T, B, drop, min_prob, loss.ptr,
                                            flag.ptr, xrow.ptr, stream()), "slk_linear_xent_grad_f16x3")
    torch.cuda.synchronize()
    xrow.get()                                                  # scratch: its contents are not asserted, its surroundings are
    assert all(i.intact() for i in ins) and lay.intact(), "an input changed"
    return g.get().reshape(M, ld), loss.get(), flag.get()


def _pair(L, lay, ld, labels, weights, T, B, drop, min_prob):
    """slk_linear_rowstats_f16x3, then slk_softmax_xent_grad_f32 in place: what the two passes replace."""
    import torch
    from sloika_amd import _lib
    M = T * B
    g, loss, flag, stats = _Out(M * ld), _Out(M), _Out(M), _Out(2 * M)
    ins = [_In(labels), _In(weights)]
    _lib.check(L.slk_linear_rowstats_f16x3(*lay.args(), g.ptr, ld, M, lay.K, lay.N, stats.ptr, stream()), "slk_linear_rowstats_f16x3")
    _lib.check(L.slk_softmax_xent_grad_f32(g.ptr, ld, stats.ptr, ins[0].ptr, ins[1].ptr, T, B, lay.N, drop, min_prob, loss.ptr, flag.ptr,
                                           stream()), "slk_softmax_xent_grad_f32")
    torch.cuda.synchronize()
    return g.get().reshape(M, ld), loss.get(), flag.get()


# ------------------------------------------------------------------------------------------------------------ checks
def _check_errors(tag, what, got, ref, y, w, dl, cap):
    """Rows with w' > 0: the error in units of w' against BOUND on the yardstick y (plus 2 dl) and against the cap (per row, in the
    same units)."""
    ok = w > 0
    if not ok.any():
        print("%s %s: no row with weight" % (tag, what))
        return
    err = rx.row_error(got, ref, w)
    bound, cap = np.broadcast_to(BOUND[what][0] * y + BOUND[what][1] + 2.0 * dl, err.shape), np.broadcast_to(cap, err.shape)
    worst = int(np.argmax(np.where(ok, err / bound, -1.0)))
    print("%s %s: error %.3e of w' (row %d), yardstick %.3e, ratio %.2f, bound %.3e, cap %.3e" %
          (tag, what, err[worst], worst, y, err[ok].max() / y if y > 0 else np.inf, bound[worst], cap[worst]))
    assert np.isfinite(np.asarray(got)[ok]).all(), "%s %s: not finite" % (tag, what)
    assert (err[ok] <= bound[ok]).all(), "%s %s: row %d off by %.3e of w'" % (tag, what, worst, err[worst])
    assert (err[ok] <= cap[ok]).all(), "%s %s: beyond the suite's cap" % (tag, what)


def _yardstick(yard, ref):
    """The case's largest float32 error, in units of w', of the gradient and of the loss rows."""
    ok = ref.w > 0
    return (float(rx.row_error(yard.g, ref.g, ref.w)[ok].max(initial=0.0)), float(rx.row_error(yard.loss, ref.loss, ref.w)[ok].max(initial=0.0)))


def _check_head(tag, got, ref, y, T, B, N, drop, dl=0.0, flag_rows=None):
    g, loss, flag = got
    M, w = T * B, ref.w
    t = np.arange(M) // B
    counted = (t >= drop) & (t < T - drop)
    # exact zeros
    assert not (g[:, N:] != 0.0).any(), tag + ": columns N .. ld-1 are not zero"
    assert not (g[w == 0] != 0.0).any(), tag + ": gradient in a dropped or weightless row"
    assert not (loss[w == 0] != 0.0).any() and not (flag[~counted] != 0.0).any(), tag + ": loss or flag outside the counted rows"
    # flags
    rows = counted if flag_rows is None else counted & flag_rows
    one = np.float32(1) / (np.float32(T - 2 * drop) * np.float32(B))
    want = np.where(ref.flag > 0, one, np.float32(0)).astype(np.float32)
    print("%s flags: %d of %d counted rows compared, %d correct" % (tag, rows.sum(), counted.sum(), (want[rows] > 0).sum()))
    assert np.array_equal(flag[rows], want[rows]), "%s: flags differ in rows %s" % (tag, np.flatnonzero(rows & (flag != want))[:8])
    assert np.isin(flag, (np.float32(0), one)).all(), tag + ": a flag that is neither 0 nor 1 / count"
    if flag_rows is not None:
        assert rows.sum() >= 0.9 * counted.sum(), tag + ": fewer than 90 % of the rows have a decided maximum"
    # errors
    _check_errors(tag, "gradient", g[:, :N], ref.g, y[0], w, dl, CAP)
    _check_errors(tag, "loss", loss, ref.loss, y[1], w, dl, CAP * ref.loss.max() / np.where(w > 0, w, 1.0))
    # sum_j g_j = coef (sum p - 1)
    total = np.abs(g[:, :N].astype(np.float64).sum(axis=1))
    ok = w > 0
    print("%s row sums: %.3e of w' at the most, allowed %.3e" % (tag, (total[ok] / w[ok]).max(initial=0.0), N * 2.0 ** -23))
    assert (total[ok] <= N * 2.0 ** -23 * w[ok]).all(), tag + ": a row's gradient does not sum to zero"


def _logit_error(scale):
    return 6e-7 * scale.max(axis=1) + 1e-6


def _decided(h, ties, regime, dl):
    """Rows whose first maximum is the same column in any arithmetic within dl of float64: the top-two gap, the duplicate of a tied
    pair set aside, exceeds 2 dl; every row of "flat" (W = 0)."""
    if regime == "flat":
        return np.ones(len(dl), bool)
    keep = np.setdiff1d(np.arange(h.logits.shape[1]), [c for _, _, c in ties])
    return rx.top_two_gap(h.logits[:, keep]) > 2.0 * dl


def _yard_from_x(h, labels, weights, T, B, N, drop, min_prob):
    """The float32 yardstick of a from-x case: the float32 head on the float64 logits rounded once, against the float64 head on the
    same -- the arithmetic of the head alone; the product's share of the error is the 2 w' dl term."""
    l32 = h.logits.astype(np.float32)
    mx, inv = rx.stats_f64(l32)
    args = (l32, l32.max(axis=1), inv.astype(np.float32), labels, weights, T, B, N, drop, min_prob)
    return _yardstick(rx.head_f32(*args), rx.head_f64(*args))


# ------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("shape,N,ldmode,shift,regime,min_prob", A_CASES)
def test_in_place_on_given_logits(shape, N, ldmode, shift, regime, min_prob):
    need_gpu()
    from sloika_amd import _lib
    T, B, drop = shape
    l, labels, weights = rx.case(_seed(shape, N, regime), T, B, N, regime, min_prob, drop)
    mx, inv = l.max(axis=1), rx.stats_f64(l)[1].astype(np.float32)
    args = (l, mx, inv, labels, weights, T, B, N, drop, min_prob)
    ref, yard = rx.head_f64(*args), rx.head_f32(*args)
    assert np.isfinite(ref.g).all() and np.isfinite(ref.loss).all()
    got = _in_place(_lib.lib(), l, _ld(N, ldmode), shift, mx, inv, labels, weights, T, B, N, drop, min_prob)
    _check_head("in place", got, ref, _yardstick(yard, ref), T, B, N, drop)


# ------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shape,N,ldmode,K,pad,regime,min_prob", B_CASES)
def test_two_passes_from_x(shape, N, ldmode, K, pad, regime, min_prob):
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, drop = shape
    ld = _ld(N, ldmode)
    x, W, b, labels, weights, ties = rx.case_x(_seed(shape, N, regime) + K, T, B, N, K, regime, min_prob, drop)
    lay = _Layer(L, x, W, b, K + 3 if pad else K)
    got = _two_pass(L, lay, ld, labels, weights, T, B, drop, min_prob)
    # (i) the pair it replaces, bit for bit: gradient with its padding columns, loss rows, flag rows
    pair = _pair(L, lay, ld, labels, weights, T, B, drop, min_prob)
    for name, a, c in zip(("gradient", "loss rows", "flag rows"), got, pair):
        assert a.tobytes() == c.tobytes(), "two passes and the in-place pair differ in the %s" % name
    # (ii) the float64 head from x, W, b
    h = rx.head_from_x_f64(x, W, b, labels, weights, T, B, drop, min_prob, ties)
    assert np.isfinite(h.g).all() and np.isfinite(h.loss).all()
    dl = _logit_error(h.scale)
    _check_head("two passes", got, h, _yard_from_x(h, labels, weights, T, B, N, drop, min_prob), T, B, N, drop, dl,
                _decided(h, ties, regime, dl))
    # the constructed ties: duplicated weight rows give the same logit to the last bit, the first of the pair is the maximum
    count = np.float32(T - 2 * drop) * np.float32(B)
    for row, a, c in ties:
        assert got[2][row] == (np.float32(1) / count if labels[row] == a else np.float32(0)), (row, a, c, int(labels[row]))


# ------------------------------------------------------------------------------------------------------------- C
def _check_eval(tag, loss, flag, ref_loss, ref_flag, y, dl, flag_rows):
    one = np.ones(len(loss))
    print("%s flags: %d of %d rows compared, %d correct" % (tag, flag_rows.sum(), len(loss), ref_flag[flag_rows].sum()))
    assert np.array_equal(flag[flag_rows], ref_flag[flag_rows]) and np.isin(flag, (0, 1)).all(), tag + ": flags"
    assert flag_rows.sum() >= 0.9 * len(loss)
    _check_errors(tag, "loss", loss, ref_loss, y, one, dl, CAP * ref_loss.max())


@pytest.mark.parametrize("shape,N,ldmode,shift,regime", C_LOGITS)
def test_validation_on_given_logits(shape, N, ldmode, shift, regime):
    import torch
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, _ = shape
    M, ld = T * B, _ld(N, ldmode)
    l, labels, _ = rx.case(_seed(shape, N, regime), T, B, N, regime, 0.0, 0)
    mx, inv = l.max(axis=1), rx.stats_f64(l)[1].astype(np.float32)
    logits = _Out(M * ld, shift=shift, init=_padded(l, ld))
    loss, flag = _Out(M), _Out(M, np.int32)
    ins = [_In(np.stack([mx, inv], axis=1).astype(np.float32)), _In(labels)]
    _lib.check(L.slk_softmax_xent_eval_f32(logits.ptr, ld, ins[0].ptr, ins[1].ptr, T, B, N, loss.ptr, flag.ptr, stream()), "eval")
    torch.cuda.synchronize()
    assert logits.untouched() and all(i.intact() for i in ins), "the logits or an input changed"
    ref_loss, ref_flag = rx.eval_f64(l, labels, N, mx, inv)
    y = float(np.abs(rx.eval_f32(l, labels, N, mx, inv)[0] - ref_loss).max())
    _check_eval("validation on logits", loss.get(), flag.get(), ref_loss, ref_flag, y, 0.0, np.ones(M, bool))


@pytest.mark.parametrize("shape,N,K,pad,regime", C_FROM_X)
def test_validation_from_x(shape, N, K, pad, regime):
    import torch
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, _ = shape
    M = T * B
    x, W, b, labels, weights, ties = rx.case_x(_seed(shape, N, regime) + K, T, B, N, K, regime, 0.0, 0)
    lay = _Layer(L, x, W, b, K + 3 if pad else K)
    loss, flag, ins = _Out(M), _Out(M, np.int32), _In(labels)
    _lib.check(L.slk_linear_xent_eval_f16x3(*lay.args(), K, N, ins.ptr, T, B, loss.ptr, flag.ptr, stream()), "eval from x")
    torch.cuda.synchronize()
    assert ins.intact() and lay.intact(), "an input changed"
    h = rx.head_from_x_f64(x, W, b, labels, weights, T, B, 0, 0.0, ties)
    ref_loss, ref_flag = rx.eval_f64(h.logits, labels, N)
    l32 = h.logits.astype(np.float32)
    mx, inv = l32.max(axis=1), rx.stats_f64(l32)[1].astype(np.float32)
    yard = float(np.abs(rx.eval_f32(l32, labels, N, mx, inv)[0] - rx.eval_f64(l32, labels, N, mx, inv)[0]).max())
    dl = _logit_error(h.scale)
    got_flag = flag.get()
    _check_eval("validation from x", loss.get(), got_flag, ref_loss, ref_flag, yard, dl, _decided(h, ties, regime, dl))
    for row, a, c in ties:
        assert got_flag[row] == (1 if labels[row] == a else 0), (row, a, c, int(labels[row]))


# ------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("K,N,ldmode", [(48, 192, "64"), (65, 192, "64"), (80, 192, "64"), (129, 192, "64"), (96, 2049, "N"),
                                        (96, 192, "64+1"), (96, 65, "64+1")],
                         ids=["K48", "K65", "K80", "K129", "N2049", "N192-ld257", "N65-ld129"])
def test_refusals_leave_every_output_alone(K, N, ldmode):
    import torch
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B = 5, 7
    M = T * B
    ld = (N + 63) // 64 * 64 + 1 if ldmode == "64+1" else _ld(N, ldmode)
    rs = np.random.RandomState(K + N)
    lay = _Layer(L, rs.normal(size=(M, K)).astype(np.float32), (rs.normal(size=(N, K)) * 0.3).astype(np.float32),
                 rs.normal(size=N).astype(np.float32), K)
    labels, weights = _In(rs.randint(0, N, size=M).astype(np.int32)), _In(np.ones(M, np.float32))
    g, loss, flag, xrow, iflag = _Out(M * ld), _Out(M), _Out(M), _Out(4 * M), _Out(M, np.int32)
    rc = L.slk_linear_xent_grad_f16x3(*lay.args(), g.ptr, ld, K, N, labels.ptr, weights.ptr, T, B, 1, 1e-30, loss.ptr, flag.ptr, xrow.ptr,
                                      stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED == _lib.SLK_ERR_UNSUPPORTED
    assert all(o.untouched() for o in (g, loss, flag, xrow))
    if ldmode != "64+1":                                         # (the validation entry has no ld)
        rc = L.slk_linear_xent_eval_f16x3(*lay.args(), K, N, labels.ptr, T, B, loss.ptr, iflag.ptr, stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and loss.untouched() and iflag.untouched()


# ------------------------------------------------------------------------------------------------------------- D
D_SHAPE, D_N, D_ROWS = (12, 11, 0), 1025, (5, 60, 131)


def _bits_equal_outside(a, c, rows):
    keep = np.setdiff1d(np.arange(len(a[1])), rows)
    return all(u[keep].tobytes() == v[keep].tobytes() for u, v in zip(a, c))


def _nonfinite_rows(got):
    return np.flatnonzero(~np.isfinite(got[0]).all(axis=1) | ~np.isfinite(got[1]))


def test_underflow_stays_in_its_row_in_place():
    """min_prob = 0 and a label 120 below the maximum: that row's loss is infinite (its gradient not finite), as the reference's own
    float32 graph gives; every other row is what it is with those labels on the maximum, to the last bit."""
    need_gpu()
    from sloika_amd import _lib
    T, B, drop = D_SHAPE
    N, rows = D_N, np.array(D_ROWS)
    l, labels, weights = rx.case(_seed(D_SHAPE, N), T, B, N, "moderate", 0.0, drop)
    top = l.argmax(axis=1)
    labels[rows] = (top[rows] + 7) % N
    l[rows, labels[rows]] = l[rows, top[rows]] - np.float32(120.0)
    weights[rows] = 1.0
    mx, inv = l.max(axis=1), rx.stats_f64(l)[1].astype(np.float32)
    moved = labels.copy()
    moved[rows] = top[rows]
    ld = _ld(N, "32")
    got = _in_place(_lib.lib(), l, ld, 0, mx, inv, labels, weights, T, B, N, drop, 0.0)
    base = _in_place(_lib.lib(), l, ld, 0, mx, inv, moved, weights, T, B, N, drop, 0.0)
    print("in place, underflow: loss of the rows", got[1][rows], "non-finite rows", _nonfinite_rows(got))
    assert not np.isfinite(got[1][rows]).any()
    assert np.array_equal(_nonfinite_rows(got), rows) and len(_nonfinite_rows(base)) == 0
    assert _bits_equal_outside(got, base, rows)


@pytest.mark.parametrize("sign", ["minus", "plus"])
def test_underflow_stays_in_its_row_two_passes(sign):
    """The same from x, by a large bias on one column with zero weights: "minus" puts the label column of the three rows 120 below
    every row's maximum (the other rows keep ordinary labels and gradients); "plus" puts another column 120 above everything, which
    every other row then has to be labelled with (their gradients are zero: the comparison is of zeros, loss rows and flags).  The
    in-place pair on the same inputs loses the same rows."""
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, drop = D_SHAPE
    N, K, rows, col = D_N, 96, np.array(D_ROWS), 500
    x, W, b, labels, weights, _ = rx.case_x(_seed(D_SHAPE, N) + K, T, B, N, K, "moderate", 0.0, drop)
    h = rx.head_from_x_f64(x, W, b, labels, weights, T, B, drop, 0.0)
    W[col] = 0.0
    weights[rows] = 1.0
    moved = labels.copy()
    if sign == "minus":
        b[col] = np.float32(h.mx.min() - 120.0)
        labels[labels == col] = col + 1
        moved = labels.copy()
        labels[rows] = col
        moved[rows] = np.delete(h.logits, col, axis=1).argmax(axis=1)[rows]
        moved[rows] += moved[rows] >= col
    else:
        b[col] = np.float32(h.mx.max() + 120.0)
        keep = labels[rows].copy()
        labels[:] = col
        moved = labels.copy()
        labels[rows] = np.where(keep == col, col + 1, keep)
    lay = _Layer(L, x, W, b, K)
    ld = _ld(N, "32")
    got, base = (_two_pass(L, lay, ld, lab, weights, T, B, drop, 0.0) for lab in (labels, moved))
    pair = _pair(L, lay, ld, labels, weights, T, B, drop, 0.0)
    print("two passes, underflow (%s): loss of the rows" % sign, got[1][rows], "non-finite rows", _nonfinite_rows(got))
    assert not np.isfinite(got[1][rows]).any()
    assert np.array_equal(_nonfinite_rows(got), rows) and len(_nonfinite_rows(base)) == 0
    assert np.array_equal(_nonfinite_rows(pair), rows)
    assert _bits_equal_outside(got, base, rows)
    if sign == "minus":
        assert np.abs(base[0]).max() > 0 and (base[2] > 0).any() and (base[2] == 0).any()
