"""Every reverse-scan kernel of the training step against a float64 recursion of its own (tests/ref_reverse_scans.py, pinned to the
training oracle by tests/test_ref_reverse_scans.py), through the C ABI:

    slk_gru_backward_f32 (its three kernels, see KERNEL), slk_gru_backward16_f32, slk_gru_backward16_dx_f32,
    slk_lstm_gates_f32, slk_lstm_backward_f32, slk_lstm_backward16_f32

at every width include/sloika_amd.h lists for the entry, the shapes of SHAPES, both directions (inside each case) and the regimes of
ref_reverse_scans.REGIMES (each its own id), the Gru entries also with a layer output h that is off by 1e-5 (NOISY_H).  Inputs are
a consistent forward pass made in float64 and rounded to float32 once; the reference runs on those float32 values, so kernel and
reference differ by the kernel's arithmetic only.

What is asserted: outputs finite, nothing written outside them, input rows and the canaries between them untouched; for EVERY chunk
the error over its T steps and columns, relative to that chunk's own largest reference entry (da, dsum, dx, dpeep[b]) or absolute
(gates, cell), at most BOUND[0] * yardstick + BOUND[1] -- the yardstick being the largest such error, over the chunks of the same
case, of the same recursion in plain float32 (y32: the float32 kernels) or float32 with 22-bit product operands (y22: the fp16-split
kernels), evaluated here on the very inputs of the case (a single chunk's own yardstick is one draw of rounding errors, ten times
below the case's worst often enough; the largest over the case is what the arithmetic costs) -- and, as before, at most what the
suite already demanded of the kernel (CAP).  rh is the float32 product r * h_prev bit for bit; a chunk without gradient comes back exactly zero.

Run time: the float64 and yardstick loops are numpy, O(T B n^2) and a few hundred Python steps per case, so the longest shape,
(200, 33), runs at the widths of LONG only (the smallest, the largest and one in between per entry).  "trained" cases run the
table's shapes in full except where TRAINED_LONG gives another shape for (200, 33), with the measured figure that rules it out;
the ids carry the shape that runs.  Lstm cases of the shapes in NO_PEEP run without peepholes.  The
regimes that differ from "moderate" only in dy or the recurrent weights are not repeated for slk_lstm_gates_f32, which reads neither.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest

from tests import ref_reverse_scans as rr
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (2, 3), (23, 9), (61, 5), (200, 33), (3, 261)]
STRIDED = (23, 9)                                        # rows of dy / hprev / h further apart than n, canaries between them
NO_PEEP = {(1, 5), (61, 5)}
GUARD = 64                                               # floats of canary before and behind every output

GRU_REGIMES = rr.REGIMES + (rr.NOISY_H,)
GRU_F32 = [16, 32, 48, 64, 96, 112, 128, 144]
GRU_16 = [16, 32, 48, 64, 80, 96, 112, 128]
GRU_DX = [(16, 16), (32, 64), (48, 16), (64, 64), (80, 48), (96, 96), (96, 32), (96, 80)]           # (n, insize)
LSTM_F32 = [16, 32, 48, 64, 96, 128]
LSTM_16 = [16, 32, 48, 64]
GATES = [16, 20, 32, 48, 64, 96, 128]
LONG = {"gru_f32": {16, 96, 144}, "gru_f32_shifted": {16, 96, 144}, "gru16": {16, 80, 128}, "gru16_dx": {(16, 16), (64, 64), (96, 96)},
        "lstm_f32": {16, 64, 128}, "lstm16": {16, 48, 64}, "gates": {16, 20, 128}}
#: what the suite already demands of a kernel, of a chunk's top (test_gpu_gru_bwd16.py: 5e-5, 1e-4 with large weights;
#: test_gpu_train.py::test_gru_backward_kernels_agree: 1e-4; test_gpu_lstm_bwd16.py: 3e-5)
CAP = {"gru_f32": 1e-4, "gru_f32_shifted": 1e-4, "gru16": 5e-5, "gru16_dx": 5e-5, "lstm16": 3e-5}


#: The "trained" regime at (200, 33).  Sixty weights of 4.5 to 6 make the Gru reverse recursion expand: measured on the float64
#: reference (these seeds, both directions alike) its largest entry is 2e+2 .. 3e+9 after 23 steps and 1e+5 .. 6e+27 after 61, with
#: yardsticks y32 / y22 of 1.5e-6 .. 1.5e-5 -- all of that runs.  A combination is replaced where the float64 reference itself goes
#: beyond 1e+30 (float32 ends at 3e+38 and the products on the way need headroom) or where the yardstick alone is beyond a quarter of
#: the suite's cap (1e-4 for the Gru with large weights, 3e-5 for the Lstm fp16-split scan), i.e. where plain float32 on the CPU
#: would not pass.  None where even the replacement is ruled out.  The Lstm scan does not expand at n >= 48 (top 4 .. 90 after 200
#: steps, yardsticks 1.1e-6 .. 2.0e-6) and runs (200, 33) as it stands.
TRAINED_LONG = {
    ("gru", 16): None,           # (200, 33): top 4.9e+89;  (61, 33): top 4.8e+27, y32 3.0e-4, y22 2.5e-4
    ("gru", 64): (61, 33),       # (200, 33): top 5.2e+35;  (61, 33): top 1.9e+12, y32 2.0e-5, y22 2.3e-5
    ("gru", 80): (61, 33),       # (200, 33): top 6.9e+26, y32 5.7e-5, y22 2.8e-5;  (61, 33): top 9.7e+8, y32 1.2e-5, y22 1.6e-5
    ("gru", 96): (61, 33),       # (200, 33): top 9.2e+25, y32 1.7e-5, y22 3.1e-5;  (61, 33): top 8.8e+8, y32 9.3e-6, y22 1.2e-5
    ("gru", 128): (61, 33),      # (200, 33): top 9.4e+19, y32 8.8e-5, y22 2.5e-4;  (61, 33): top 9.0e+5, y32 1.2e-5, y22 8.6e-6
    ("gru", 144): (61, 33),      # (200, 33): top 3.5e+18, y32 7.0e-5;  (61, 33): top 4.8e+4, y32 9.5e-6
    ("lstm", 16): (61, 33),      # (200, 33): top 1.6e+5, y32 2.9e-5, y22 3.6e-5;  (61, 33): top 1.1e+2, y32 5.2e-6, y22 1.9e-6
}
#: the kernel an entry reaches at a width (sloika_amd/csrc/train.hip: slk_gru_backward_f32; gru_backward_mfma.hip: its dispatch), named
#: in every message.  Through the C ABI the LDS-DMA kernel is reachable at 128 and 144 only: below that aligned rows go to the MFMA one.
KERNEL = {"gru_f32": lambda n: "gru_backward_mfma_kernel" if n <= 112 else "gru_backward_dma_kernel",
          "gru_f32_shifted": lambda n: "gru_backward_kernel", "gru16": lambda n: "gru_bwd16_kernel",
          "gru16_dx": lambda n: "gru_bwd16_kernel<DX>", "lstm_f32": lambda n: "lstm_backward_kernel",
          "lstm16": lambda n: "lstm_bwd16_kernel", "gates": lambda n: "lstm_gates_kernel"}


def _cases(entry, widths, regimes=rr.REGIMES):
    out = []
    for w in widths:
        for T, B in SHAPES:
            if (T, B) == (200, 33) and w not in LONG[entry]:
                continue
            for regime in regimes:
                n, insize = w if isinstance(w, tuple) else (w, 0)
                t, b = T, B
                if regime == "trained" and (T, B) == (200, 33):
                    shape = TRAINED_LONG.get((entry[:3] if entry.startswith("gru") else "lstm", n), (T, B))
                    if shape is None:
                        continue
                    t, b = shape
                out.append(pytest.param(entry, n, insize, t, b, regime,
                                        id="%s-n%d%s-T%d-B%d-%s" % (entry, n, "-i%d" % insize if insize else "", t, b, regime)))
    return out


def _ordered(params):
    """Cases on the same inputs next to each other: the float64 reference of a case is computed once (the cache below)."""
    return sorted(params, key=lambda p: (p.values[1], p.values[3], p.values[4], p.values[5], p.values[0], p.values[2]))


def _seed(n, T, B, regime):
    return 1000 * n + 7 * T + B + 100000 * GRU_REGIMES.index(regime)


# ----------------------------------------------------------------------------------------------------------- buffers
class _Rows:
    """A float32 matrix on the device with its rows `ld` floats apart, NaN between the rows and around them, its first element
    `shift` floats past a 16-byte boundary."""

    def __init__(self, a, ld, shift=0):
        M, n = a.shape
        self.host = np.full(M * ld + 8, np.nan, np.float32)
        self.host[shift:shift + M * ld].reshape(M, ld)[:, :n] = a
        self.t, self.ld = dev(self.host), ld
        self.ptr = self.t.data_ptr() + 4 * shift

    def intact(self):
        return np.array_equal(self.t.cpu().numpy(), self.host, equal_nan=True)


class _Out:
    """M rows of `cols` floats, `ld` apart, NaN everywhere before the call; get() checks that only the rows' own floats were written."""

    def __init__(self, M, cols, ld=None):
        import torch
        self.M, self.cols, self.ld = M, cols, ld or cols
        self.t = torch.full((2 * GUARD + M * self.ld,), float("nan"), dtype=torch.float32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def get(self):
        a = self.t.cpu().numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + self.M * self.ld:]).all(), "written outside the output"
        rows = a[GUARD:GUARD + self.M * self.ld].reshape(self.M, self.ld)
        assert np.isnan(rows[:, self.cols:]).all(), "written between the output rows"
        assert np.isfinite(rows[:, :self.cols]).all(), "output not finite"
        return rows[:, :self.cols]


# ------------------------------------------------------------------------------------------------------- comparison
def _judge(label, what, got, ref, yard, T, B, cap=None, relative=True):
    """Every chunk of `got` within BOUND of the reference, the yardstick being the worst chunk of `yard` in the same normalisation."""
    measure = rr.chunk_error if relative else rr.chunk_abs_error
    err, y = measure(got, ref, T, B), float(measure(yard, ref, T, B).max())
    bound = rr.BOUND[0] * y + rr.BOUND[1]
    worst = int(np.argmax(err))
    print("REVSCAN %s %s err %.3e yardstick %.3e bound %.3e ratio %.2f chunk %d" % (label, what, err[worst], y, bound,
                                                                                  err[worst] / max(y, 2.0 ** -24), worst))
    assert (err <= bound).all(), "%s %s: chunk %d is %.3e from the float64 recursion, the yardstick %.3e allows %.3e" % (
        label, what, worst, err[worst], y, bound)
    if cap is not None:
        assert (err <= cap).all(), "%s %s: %.3e is beyond the suite's cap %.1e" % (label, what, err[worst], cap)
    zero = np.abs(np.asarray(ref).reshape(T, B, -1)).max(axis=(0, 2)) == 0.0
    assert not np.asarray(got).reshape(T, B, -1)[:, zero].any(), "%s %s: a chunk without gradient is not exactly zero" % (label, what)


# -------------------------------------------------------------------------------------------------------------- Gru
class _Lazy(dict):
    """Inputs and float64 reference of one case, the yardsticks filled in when an entry first asks for them."""


@functools.lru_cache(maxsize=4)
def _gru_reference(n, T, B, regime, reverse):
    c = _Lazy(rr.gru_case(_seed(n, T, B, regime), T, B, n, regime, reverse))
    if regime.startswith("saturated"):
        rr.assert_gru_saturated(c)
    c["da"], c["rh"] = rr.gru_reverse_scan(c["dy"], c["z"], c["r"], c["c"], c["h_prev"], c["sW"], c["sW2"], T, B, reverse)
    assert np.isfinite(c["da"]).all() and np.abs(c["da"]).max() < 1e30
    return c


def _gru_yardstick(c, T, B, reverse, bits):
    key = "y%s" % bits
    if key not in c:
        c[key] = rr.gru_reverse_scan_f32(c["dy"], c["z"], c["r"], c["h"], c["h_prev"], c["sW"], c["sW2"], T, B, reverse, bits)[0]
    return c[key]


DACT = {"tanh": lambda y: 1.0 - y * y, "elu": lambda y: np.where(y > 0, 1.0, y + 1.0), "relu": lambda y: (y > 0) * 1.0}


@pytest.mark.parametrize("entry,n,insize,T,B,regime", _ordered(
    _cases("gru_f32", GRU_F32, GRU_REGIMES) + _cases("gru_f32_shifted", GRU_F32, GRU_REGIMES) + _cases("gru16", GRU_16, GRU_REGIMES) +
    _cases("gru16_dx", GRU_DX, GRU_REGIMES)))
def test_gru_reverse_scan(entry, n, insize, T, B, regime):
    need_gpu()
    from sloika_amd import _lib, activation
    L = _lib.lib()
    strided = (T, B) == STRIDED
    M = T * B
    shift = 1 if entry == "gru_f32_shifted" else 0       # dy off the 16-byte grid: the plain kernel, at every width
    pad = (3 if shift else 4) if strided else 0
    bits = None if entry.startswith("gru_f32") else 22
    # NOISY_H: the caps were set on outputs of two kernels fed the SAME h, where what the noise in h costs cancels; here it does not.
    # Its only bound is four times a yardstick made from the same noisy h with the clamp (1.7e-5 .. 6.4e-4 of a chunk's top): in this
    # regime the test sees whether the recovered candidate is clamped, and little else.
    cap = 1e-4 if regime == "trained" else None if regime == rr.NOISY_H else CAP[entry]
    for reverse in (False, True):
        label = "%s (%s) n=%d T=%d B=%d %s rev=%d" % (entry, KERNEL[entry](n), n, T, B, regime, reverse)
        c = _gru_reference(n, T, B, regime, reverse)
        dy, hp, h = _Rows(c["dy"], n + pad, shift), _Rows(c["h_prev"], n + pad), _Rows(c["h"], n + pad)
        zr, sW, sW2 = dev(np.concatenate([c["z"], c["r"]], axis=1)), dev(c["sW"]), dev(c["sW2"])
        da, rh = _Out(M, 3 * n), _Out(M, n)
        if entry == "gru16_dx":
            rs = np.random.RandomState(n + insize + T)
            iW = (2.0 * rs.normal(size=(3 * n, insize)) / np.sqrt(n + insize)).astype(np.float32)
            dact = [None, "tanh", "elu", "relu"][(n // 16 + reverse + GRU_REGIMES.index(regime)) % 4]
            yb = _Rows(np.tanh(rs.normal(size=(M, insize))).astype(np.float32), insize + (5 if strided else 0))
            dx = _Out(M, insize, insize + 3)                 # rows of dx need not be dense
            iWd = dev(iW)
            rc = L.slk_gru_backward16_dx_f32(dy.ptr, dy.ld, hp.ptr, hp.ld, zr.data_ptr(), h.ptr, h.ld, sW.data_ptr(), sW2.data_ptr(),
                                             iWd.data_ptr(), da.ptr, rh.ptr, dx.ptr, dx.ld, T, B, n, insize, int(reverse), 1, 2,
                                             yb.ptr if dact else None, yb.ld, activation.act_id(getattr(activation, dact)) if dact else 0,
                                             stream())
        else:
            name = "slk_gru_backward16_f32" if entry == "gru16" else "slk_gru_backward_f32"
            rc = getattr(L, name)(dy.ptr, dy.ld, hp.ptr, hp.ld, zr.data_ptr(), h.ptr, h.ld, sW.data_ptr(), sW2.data_ptr(), da.ptr, rh.ptr,
                                  T, B, n, int(reverse), 1, 2, stream())
        assert rc == 0, label
        got_da, got_rh = da.get(), rh.get()
        assert dy.intact() and hp.intact() and h.intact()
        yard = _gru_yardstick(c, T, B, reverse, bits)
        _judge(label, "da", got_da, c["da"], yard, T, B, cap)
        np.testing.assert_array_equal(got_rh, c["r"] * c["h_prev"])
        assert np.abs(got_rh - c["rh"]).max() <= 2.0 ** -24
        if entry == "gru16_dx":
            assert yb.intact()
            fun = DACT[dact](yb.host[:M * yb.ld].reshape(M, yb.ld)[:, :insize].astype(np.float64)) if dact else 1.0
            ref_dx = (c["da"] @ iW.astype(np.float64)) * fun
            yard_dx = rr.product_f32(yard, iW, 22) * np.asarray(fun, np.float32)
            got_dx = dx.get()
            _judge(label, "dx", got_dx, ref_dx, yard_dx, T, B)
            # ... and as before: float32-grade against the float64 product of the kernel's OWN da
            own = (got_da.astype(np.float64) @ iW.astype(np.float64)) * fun
            e = rr.chunk_error(got_dx, own, T, B)
            print("REVSCAN %s dx-of-own-da err %.3e" % (label, e.max()))
            assert (e <= 2e-6).all(), float(e.max())


# ------------------------------------------------------------------------------------------------------------- Lstm
@functools.lru_cache(maxsize=4)
def _lstm_reference(n, T, B, regime, reverse, peepholes):
    c = _Lazy(rr.lstm_case(_seed(n, T, B, regime), T, B, n, regime, reverse, peepholes))
    if regime == "saturated":
        rr.assert_lstm_saturated(c)
    c["dsum"], c["dpeep"] = rr.lstm_reverse_scan(c["dy"], c["gates"], c["cell"], c["sW"], c["peep"], T, B, reverse)
    assert np.isfinite(c["dsum"]).all() and np.abs(c["dsum"]).max() < 1e30
    return c


@pytest.mark.parametrize("entry,n,insize,T,B,regime", _ordered(_cases("lstm_f32", LSTM_F32) + _cases("lstm16", LSTM_16)))
def test_lstm_reverse_scan(entry, n, insize, T, B, regime):
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    strided, peepholes = (T, B) == STRIDED, (T, B) not in NO_PEEP
    M = T * B
    bits = None if entry == "lstm_f32" else 22
    for reverse in (False, True):
        label = "%s (%s) n=%d T=%d B=%d %s rev=%d peep=%d" % (entry, KERNEL[entry](n), n, T, B, regime, reverse, peepholes)
        c = _lstm_reference(n, T, B, regime, reverse, peepholes)
        dy = _Rows(c["dy"], n + (4 if strided else 0))
        gates, cell, sW = dev(c["gates"]), dev(c["cell"]), dev(c["sW"])
        peep = dev(c["peep"]) if peepholes else None
        dsum, dpeep = _Out(M, 4 * n), _Out(B, 3 * n)
        name = "slk_lstm_backward16_f32" if entry == "lstm16" else "slk_lstm_backward_f32"
        rc = getattr(L, name)(dy.ptr, dy.ld, gates.data_ptr(), cell.data_ptr(), sW.data_ptr(), peep.data_ptr() if peepholes else None,
                              dsum.ptr, dpeep.ptr, T, B, n, int(reverse), 1, 2, stream())
        assert rc == 0, label
        got, gotp = dsum.get(), dpeep.get()
        assert dy.intact()
        key = "y%s" % bits
        if key not in c:
            c[key] = rr.lstm_reverse_scan(c["dy"], c["gates"], c["cell"], c["sW"], c["peep"], T, B, reverse, np.float32, bits)
        _judge(label, "dsum", got, c["dsum"], c[key][0], T, B, CAP.get(entry))
        _judge(label, "dpeep", gotp, c["dpeep"], c[key][1], 1, B, CAP.get(entry))


@pytest.mark.parametrize("entry,n,insize,T,B,regime", _cases("gates", GATES, ("moderate", "saturated")))
def test_lstm_cell_scan(entry, n, insize, T, B, regime):
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    peepholes = (T, B) not in NO_PEEP
    M = T * B
    for reverse in (False, True):
        label = "%s n=%d T=%d B=%d %s rev=%d peep=%d" % (entry, n, T, B, regime, reverse, peepholes)
        c = rr.lstm_case(_seed(n, T, B, regime), T, B, n, regime, reverse, peepholes)
        if regime == "saturated":
            rr.assert_lstm_saturated(c)
        ref_g, ref_c = rr.lstm_cell_scan(c["sum"], c["peep"], T, B, reverse)
        y_g, y_c = rr.lstm_cell_scan(c["sum"], c["peep"], T, B, reverse, np.float32)
        sm, peep = dev(c["sum"]), dev(c["peep"]) if peepholes else None
        gates, cell = _Out(M, 4 * n), _Out(M, n)
        rc = L.slk_lstm_gates_f32(sm.data_ptr(), peep.data_ptr() if peepholes else None, gates.ptr, cell.ptr, T, B, n, int(reverse), stream())
        assert rc == 0, label
        _judge(label, "gates", gates.get(), ref_g, y_g, T, B, relative=False)
        _judge(label, "cell", cell.get(), ref_c, y_c, T, B, relative=False)
