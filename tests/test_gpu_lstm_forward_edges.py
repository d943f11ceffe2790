"""The forward Lstm kernels -- csrc/lstm_fused16.hip (slk_lstm_fused16_f32), csrc/lstm_scan16.hip (slk_lstm_scan16_f32),
csrc/lstm_mfma.hip and the portable kernel of csrc/recurrent.hip (slk_lstm_recurrent_f32, slk_lstm_recurrent_ragged_f32) and
slk_lstm_f32 -- through the C ABI, against a float64 recursion of their own (tests/ref_lstm_forward.py, pinned on the CPU by
tests/test_ref_lstm_forward.py) at every time and batch edge.

What is asserted of every launch (`rl.check`): for EVERY chunk, over that chunk's own steps, the largest absolute error of h is at
most BOUND[0] * yard + BOUND[1] -- yard being the largest such error, over the chunks of the case, of the same recursion in the
arithmetic include/sloika_amd.h promises for the entry (y22: float32 with 22-bit product operands, for the fp16-split kernels; y32:
float32, for the others), evaluated on the very inputs of the case -- and at most the 2e-5 the suite already demanded.  Every figure
is printed on an `LSTMFWD ...` line before it is asserted.

How every launch is set up: outputs start as a NaN of a fixed bit pattern with 64 guard floats in front of and behind them, rows
ld floats apart with the pattern in the gaps; x rows are ldx = I + 4 apart with NaN in the gaps; every x or vW row at t >= lens[b] is
NaN (the layers hand the kernels uninitialised rows there: a kernel that reads one of them into a product loses the chunk); after
the call the guards, the gaps and every output row past a chunk's end hold the bits they held before, and the inputs are unchanged.
The lengths of rl.EDGE_T and rl.MFMA_T are laid around the constants the kernel sources declare (rl.declared_geometry(), tied to
the tables in tests/test_ref_lstm_forward.py), which every test here asserts first: a kernel change that moves the edges fails there.

References and yardsticks are made once per case and shared (rl.layer_case, rl.scan_case).

Worst err / (yard + BOUND[1] / BOUND[0]) per kernel, as printed by test_recorded_figures on an MI355X (the bound is 4):
    fused16<1> 2.66 ((32, 32) trained, T = 5)   fused16<2> 1.21   scan16<64> 1.36   scan16<128> 1.09
    mfma 1.28   generic 1.64   gemm+scan 1.00
and the largest yardsticks: y22 moderate 1.30e-6 (a mixed case), y22 trained 1.57e-6, y32 moderate 5.14e-7.  Without `trained` the
worst fused16<1> ratio is 1.46.  One finding went into the yardstick, not the bound: rl.summation_orders."""
import functools

import numpy as np
import pytest

from tests import ref_lstm_forward as rl
from tests.gpu_util import Out, dev, nan_filled, need_gpu, padded_input, stream

pytestmark = pytest.mark.gpu

DIRECTIONS = [False, True]
GEOMETRY = {"KB": 8, "fused_group": 4, "fused_ahead": 2, "scan_unroll": 4, "scan_sets": 4, "scan_ahead": 3}
ODD = dict(extra=3, lead=1)                    # rows n + 3 apart, the first one float past a 16-byte boundary


@functools.lru_cache(maxsize=None)
def _geometry_is_as_declared():
    return rl.declared_geometry() == GEOMETRY


@functools.lru_cache(maxsize=None)
def _weights(I, n, regime):
    return tuple(dev(a) for a in rl.weights(I, n, regime))


def _lib():
    need_gpu()
    from sloika_amd import _lib
    assert _geometry_is_as_declared(), rl.declared_geometry()
    return _lib.lib()


def _plan(I, n):
    from sloika_amd import activation, layers
    return layers.lstm_plan(I, n, activation.tanh, activation.sigmoid)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _label(c, kernel, extra=""):
    return "%s (%d,%d) %s T=%d B=%d rev=%d lens=%d b=%d p=%d%s" % (kernel, c["I"], c["n"], c["regime"], c["T"], c["B"], int(c["reverse"]),
                                                                  c["lens"] is not None, c["b"] is not None, c["p"] is not None, extra)


def _finish(y, inputs, c, tell, what):
    import torch
    torch.cuda.synchronize()
    for now, before in inputs:
        assert torch.equal(now.view(torch.int32), before.view(torch.int32)), what + ": an input changed"
    y.fetch().assert_untouched_outside(c["lens"] if tell else None, what)
    return y


# ------------------------------------------------------------------------------------------------- slk_lstm_fused16_f32
def fused_kernel(I):
    return "fused16<1>" if I <= 32 else "fused16<2>"


def run_fused(c, extra=0, lead=0, tell=True):
    """One slk_lstm_fused16_f32 launch of case c -> y as a fetched Out, everything outside the output verified."""
    L = _lib()
    I, n, T, B, lens = c["I"], c["n"], c["T"], c["B"], c["lens"]
    assert _plan(I, n) == "layer"
    xd = padded_input(c["x"], lens, I + 4)
    x0 = xd.clone()
    iW, sW, b, p = _weights(I, n, c["regime"])
    ld = None if lens is None or not tell else dev(np.asarray(lens, np.int32))
    y = Out(T, B, n, n + extra, lead)
    rc = L.slk_lstm_fused16_f32(xd.data_ptr(), I + 4, iW.data_ptr(), sW.data_ptr(), _ptr(b if c["b"] is not None else None),
                                _ptr(p if c["p"] is not None else None), y.ptr(), y.ld, T, B, I, n, int(c["reverse"]), 1, 2, _ptr(ld), stream())
    what = _label(c, fused_kernel(I))
    assert rc == 0, (what, rc)
    return _finish(y, [(xd, x0)], c, tell, what)


def fused_twice(c, note="", **kw):
    """The case twice: within the bound, and the second launch with the bits of the first."""
    y = run_fused(c, **kw)
    rl.check(y.values(), c, _label(c, fused_kernel(c["I"]), note), fused_kernel(c["I"]))
    again = run_fused(c, **kw)
    assert np.array_equal(y.host, again.host), _label(c, fused_kernel(c["I"]), note + ": the second launch differs")
    return y


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rl.FUSED_SHAPES)
def test_fused16_time_edges(I, n, reverse):
    """T in rl.EDGE_T (moderate), the admitted lengths of `trained` and of the mixed-magnitude x, B = 17: four full workgroups and a
    last one with a single live chunk whose dead slots re-read its rows."""
    for regime, T, mixed in rl.edge_entries(I, n):
        fused_twice(rl.layer_case(I, n, regime, T, rl.EDGE_B, reverse, None, mixed), " mixed" if mixed else "")


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rl.FUSED_SHAPES)
def test_fused16_batch_edges(I, n, reverse):
    """T = 9, every B of rl.BATCH_B: the first B chunks of one case of nine (chunks do not see each other)."""
    base = rl.layer_case(I, n, "moderate", rl.BATCH_T, max(rl.BATCH_B), reverse)
    for B in rl.BATCH_B:
        fused_twice(base.take(B))


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rl.FUSED_SHAPES)
def test_fused16_null_bias_null_peepholes_and_output_placement(I, n, reverse):
    """b = NULL, p = NULL and both (T = 9, B = 17); y one float past a 16-byte boundary with ldy = n + 3, full and ragged."""
    for bias, peep in ((False, True), (True, False), (False, False)):
        fused_twice(rl.layer_case(I, n, "moderate", rl.BATCH_T, rl.EDGE_B, reverse, None, False, bias, peep))
    for c in (rl.layer_case(I, n, "moderate", rl.BATCH_T, rl.EDGE_B, reverse, None, False),
              rl.layer_case(I, n, "moderate", rl.RAGGED_T, rl.RAGGED_B, reverse, rl.ragged_lens())):
        plain = run_fused(c)
        odd = fused_twice(c, " ldy=n+3", **ODD)
        assert np.array_equal(plain.values().view(np.uint32), odd.values().view(np.uint32))


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rl.FUSED_SHAPES)
def test_fused16_ragged(I, n, reverse):
    """T = 17, B = 17, lengths of rl.ragged_lens(): each chunk against float64 on the chunk alone, a reversed scan from the chunk's own
    last row.  Then T = 9 with every length equal to T: the bits of the call with lens = NULL."""
    fused_twice(rl.layer_case(I, n, "moderate", rl.RAGGED_T, rl.RAGGED_B, reverse, rl.ragged_lens()))
    full = rl.layer_case(I, n, "moderate", rl.BATCH_T, rl.EDGE_B, reverse, (rl.BATCH_T,) * rl.EDGE_B)
    told = fused_twice(full)
    assert np.array_equal(told.host, run_fused(full, tell=False).host), "lens = T everywhere differs from lens = NULL"


def test_fused16_long():
    I, n = rl.LONG_FUSED
    fused_twice(rl.layer_case(I, n, "moderate", *rl.LONG, False))


# ------------------------------------------------------------------------------------------------------ the scan entries
def scan_kernel(c):
    n = c["n"]
    if c["grade"] == "y22":
        return "scan16<64>" if n <= 64 else "scan16<128>"
    return "mfma" if n in rl.MFMA_SIZES and (c["act"], c["gate"]) == ("tanh", "sigmoid") else "generic"


def run_scan(c, extra=0, lead=0, ragged_entry=None):
    """One launch of case c through the entry of its grade: y22 -> slk_lstm_scan16_f32; y32 -> slk_lstm_recurrent_f32, or
    slk_lstm_recurrent_ragged_f32 where the case has lengths (or ragged_entry says so)."""
    L = _lib()
    n, T, B, lens = c["n"], c["T"], c["B"], c["lens"]
    kernel = scan_kernel(c)
    vd = padded_input(c["vW"], lens, 4 * n)
    v0 = vd.clone()
    sW, p = _weights(c["I"], n, "moderate")[1::2]
    p = p if c["p"] is not None else None
    ld = None if lens is None else dev(np.asarray(lens, np.int32))
    act, gate = rl.ACTIVATIONS[c["act"]][2], rl.ACTIVATIONS[c["gate"]][2]
    y = Out(T, B, n, n + extra, lead)
    args = (vd.data_ptr(), sW.data_ptr(), _ptr(p), y.ptr(), y.ld, T, B, n, int(c["reverse"]), act, gate)
    if kernel.startswith("scan16"):
        assert _plan(68, n) == "scan16"                               # (an input too wide for the whole-layer kernel)
        rc = L.slk_lstm_scan16_f32(*args, _ptr(ld), stream())
    else:
        if kernel == "generic" and (act, gate) == (1, 2):
            assert _plan(68, n) == "scan"                             # no fp16-split kernel takes the size
        if ld is None and ragged_entry:
            ld = dev(np.full(B, T, np.int32))
        rc = L.slk_lstm_recurrent_f32(*args, stream()) if ld is None else L.slk_lstm_recurrent_ragged_f32(*args, ld.data_ptr(), stream())
    what = _label(c, kernel)
    assert rc == 0, (what, rc)
    return _finish(y, [(vd, v0)], c, True, what)


def scan_twice(c, note="", **kw):
    kernel = scan_kernel(c)
    y = run_scan(c, **kw)
    rl.check(y.values(), c, _label(c, kernel, note), kernel)
    assert np.array_equal(y.host, run_scan(c, **kw).host), _label(c, kernel, note + ": the second launch differs")
    return y


@pytest.mark.parametrize("peep", [True, False])
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rl.SCAN_SIZES)
def test_scan16_edges(n, reverse, peep):
    """slk_lstm_scan16_f32: vW is the float32 rounding of the float64 projection, NaN in the rows past a chunk's end.  T in rl.EDGE_T at
    B = 17, every B of rl.BATCH_B at T = 9, the ragged case; the last two also with ldo = n + 3, one float off alignment."""
    for T in rl.EDGE_T:
        scan_twice(rl.scan_case(n, T, rl.EDGE_B, reverse, None, peep))
    base = rl.scan_case(n, rl.BATCH_T, max(rl.BATCH_B), reverse, None, peep)
    for B in rl.BATCH_B:
        scan_twice(base.take(B))
    ragged = rl.scan_case(n, rl.RAGGED_T, rl.RAGGED_B, reverse, rl.ragged_lens(), peep)
    for c in (base, ragged):
        plain = scan_twice(c)
        odd = scan_twice(c, " ldo=n+3", **ODD)
        assert np.array_equal(plain.values().view(np.uint32), odd.values().view(np.uint32))


def test_scan16_long():
    scan_twice(rl.scan_case(rl.LONG_SCAN, *rl.LONG, False))


STORES = [dict(extra=4, lead=0), ODD]            # 16-byte stores (rows n + 4 apart, aligned); scalar stores


@pytest.mark.parametrize("store", STORES, ids=["vector", "scalar"])
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rl.MFMA_SIZES)
def test_mfma_edges(n, reverse, store):
    """lstm_mfma_kernel through slk_lstm_recurrent_f32 / _ragged_f32, yardstick y32, in both store paths (lstm_mfma.hip:99): T in
    rl.MFMA_T at B = 17 (both slots of the DMA ring, the first refill of either, the late flush), every B of rl.BATCH_B at T = 9, and
    lengths of rl.mfma_ragged_lens() inside T = 25.  The ragged entry with every length equal to T: the bits of the other entry."""
    note = " ldo=n+%d lead=%d" % (store["extra"], store["lead"])
    for T in rl.MFMA_T:
        scan_twice(rl.scan_case(n, T, rl.EDGE_B, reverse, None, True, "y32"), note, **store)
    base = rl.scan_case(n, rl.BATCH_T, max(rl.BATCH_B), reverse, None, True, "y32")
    for B in rl.BATCH_B:
        scan_twice(base.take(B), note, **store)
    scan_twice(rl.scan_case(n, rl.MFMA_RAGGED_T, rl.RAGGED_B, reverse, rl.mfma_ragged_lens(), True, "y32"), note, **store)
    assert np.array_equal(run_scan(base, **store).host, run_scan(base, ragged_entry=True, **store).host)


def test_mfma_long():
    scan_twice(rl.scan_case(rl.LONG_MFMA, *rl.LONG, False, None, True, "y32"), **STORES[0])


@pytest.mark.parametrize("n", rl.GENERIC_SIZES)
def test_generic_kernel(n):
    """lstm_generic_kernel (sizes lstm_mfma.hip has no instantiation for) through the same two entries, yardstick y32: T in (1, 2, 9),
    B in (1, 5), a ragged batch, and one case with fair / sigmoid_pm, which no other Lstm kernel takes."""
    from sloika_amd import _lib as lib_module
    L = _lib()
    z = dev(np.zeros(4 * n * n + 8 * n, np.float32))
    assert L.slk_lstm_scan16_f32(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), n, 1, 1, n, 0, 1, 2, None,
                                 stream()) == lib_module.SLK_ERR_UNSUPPORTED          # the split scan refuses the size
    for reverse in DIRECTIONS:
        for T in rl.GENERIC_T:
            base = rl.scan_case(n, T, max(rl.GENERIC_B), reverse, None, True, "y32")
            for B in rl.GENERIC_B:
                scan_twice(base.take(B), **ODD)
        ragged = rl.scan_case(n, max(rl.GENERIC_T), max(rl.GENERIC_B), reverse, rl.GENERIC_LENS, True, "y32")
        scan_twice(ragged, extra=4)
    other = rl.scan_case(n, max(rl.GENERIC_T), max(rl.GENERIC_B), True, None, True, "y32", rl.OTHER_PAIR)
    assert scan_kernel(other) == "generic"
    scan_twice(other, " fair/sigmoid_pm", extra=4)


@pytest.mark.parametrize("n", rl.MFMA_SIZES)
def test_other_activations_take_the_generic_kernel_at_mfma_sizes(n):
    c = rl.scan_case(n, max(rl.GENERIC_T), max(rl.GENERIC_B), True, None, True, "y32", rl.OTHER_PAIR)
    assert scan_kernel(c) == "generic"
    scan_twice(c, " fair/sigmoid_pm", **ODD)


# --------------------------------------------------------------------------------------------------------- slk_lstm_f32
@pytest.mark.parametrize("I,n", rl.GEMM_SHAPES)
def test_lstm_f32_and_its_workspace(I, n):
    """Projection GEMM + scan through a workspace (yardstick y32 of the whole layer); a workspace one byte short returns
    SLK_ERR_WORKSPACE, and neither y nor the workspace is written."""
    import torch
    from sloika_amd import _lib as lib_module
    L = _lib()
    T, B = rl.BATCH_T, 5
    need = L.slk_lstm_workspace_bytes(T, B, n)
    assert need == 4 * T * B * 4 * n
    iW, sW, b, p = _weights(I, n, "moderate")
    for reverse in DIRECTIONS:
        c = rl.gemm_case(I, n, T, B, reverse)
        xd = padded_input(c["x"], None, I + 4)
        x0 = xd.clone()
        ws = dev(nan_filled(need // 4 + 64))
        w0 = ws.clone()
        y = Out(T, B, n, n + 3, 1)
        args = (xd.data_ptr(), I + 4, iW.data_ptr(), sW.data_ptr(), b.data_ptr(), p.data_ptr(), y.ptr(), y.ld, T, B, I, n, int(reverse), 1, 2)
        assert L.slk_lstm_f32(*args, ws.data_ptr(), need - 1, stream()) == lib_module.SLK_ERR_WORKSPACE
        assert L.slk_lstm_f32(*args, None, need, stream()) == lib_module.SLK_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.equal(ws.view(torch.int32), w0.view(torch.int32)), "a refused call wrote the workspace"
        assert (y.fetch().host == y.host[0]).all(), "a refused call wrote y"
        assert L.slk_lstm_f32(*args, ws.data_ptr(), need, stream()) == 0
        what = _label(c, "gemm+scan")
        _finish(y, [(xd, x0)], c, True, what)
        assert torch.equal(ws[need // 4:].view(torch.int32), w0[need // 4:].view(torch.int32)), "written past the workspace"
        rl.check(y.values(), c, what, "gemm+scan")


# ---------------------------------------------------------------------------------------------------------- figures
def test_recorded_figures():
    """The worst err / yardstick per kernel and the largest yardstick per grade and regime over the LSTMFWD lines of this run (the
    module docstring keeps the table).  A ratio above BOUND[0] has already failed its own test; here it fails once more, by name."""
    for kernel, ratio in sorted(rl.FIGURES["ratio"].items()):
        print("LSTMFWD-SUMMARY kernel %s worst ratio %.2f" % (kernel, ratio))
    for (grade, regime), y in sorted(rl.FIGURES["yard"].items()):
        print("LSTMFWD-SUMMARY yardstick %s regime %s largest %.3e" % (grade, regime, y))
    assert all(r <= rl.BOUND[0] for r in rl.FIGURES["ratio"].values()), rl.FIGURES["ratio"]
    assert all(y <= rl.ADMIT for y in rl.FIGURES["yard"].values()), rl.FIGURES["yard"]
