"""The whole-layer Gru kernels -- csrc/gru_bar16.hip with gru_bar16_body.h (four chunks per workgroup), gru_bar16d.hip (eight),
gru_bar16q.hip (sixteen), the packed stack entry and gru_scan1t.hip for the wide layers -- through the C ABI, against a float64
recursion of their own (tests/ref_gru_forward.py, pinned on the CPU by tests/test_ref_gru_forward.py) at every time and batch edge.

What is asserted of every launch (`rg.check`): for EVERY chunk, over that chunk's own steps, the largest absolute error of h (and of
the saved gates z | r) is at most BOUND[0] * y22 + BOUND[1] -- y22 being the largest such error, over the chunks of the case, of
the same recursion in float32 with 22-bit product operands, evaluated on the very inputs of the case -- and at most the 2e-5 the
suite already demanded.  Every figure is printed on a `GRUFWD ...` line before it is asserted.

How every launch is set up unless a test says otherwise: outputs start as a NaN of a fixed bit pattern with 64 guard floats in front of
and behind y and zr; x rows are ldx = I + 4 apart with NaN in the gaps; every x row at t >= lens[b] is NaN (the layers hand the
kernels uninitialised rows there: a kernel that reads one of them into a product loses the chunk); after the call the guards, the gaps
and every output row past a chunk's end hold the bits they held before, and x is unchanged.  Every test first asserts that the ring of
its plan is two projection groups as the kernel source declares them (gru_bar16_body.h:18-19, gru_bar16d.hip:57-58: GS = 4, R = 2 * GS;
gru_bar16q.hip:46-47: GS = 2, R = 2 * GS): the lengths of rg.EDGE_T are laid around those, and a kernel change that moves the edges
must fail here first (the table itself is tied to them in tests/test_ref_gru_forward.py).

References and yardsticks are made once per (shape, regime, T, direction) and shared by the plans and the tests (rg.layer_case).

The float32 scan of csrc/recurrent.hip -- gru_mfma_kernel (v_mfma_f32_4x4x1) and gru_generic_kernel behind slk_gru_recurrent_f32,
slk_gru_recurrent_f32_ex, slk_gru_recurrent_ragged_f32 and the GEMM + scan fallback of slk_gru_f32: the "scan" plan of layers.gru_plan
-- is held to the same bound with the y32 yardstick (plain float32, the worse of rg.F32_ORDERS) over vI as the float32 rounding of the
float64 projection.  Its launches: vI dense from a 16-byte boundary with NaN in every row at t >= lens[b]; h_out with guards and the NaN
pattern, rows n apart from a 16-byte boundary (16-byte stores) or n + 3 apart one float past it (scalar stores); inputs unchanged, guards,
gaps and rows past a chunk's end untouched; every launch twice, the second with the bits of the first.  The lengths of rg.F32_T are laid
around KB and the tile of four chunks as the kernel source declares them (rg.declared_f32_scan_geometry(), tied to the tables in
tests/test_ref_gru_forward.py), which every launch asserts first.

Worst err / (y32 + BOUND[1] / BOUND[0]) per kernel of the float32 scan, as printed by test_recorded_figures on an MI355X (the bound is 4):
    f32 mfma<4 waves> 1.53 (n = 32, T = 17, B = 17, forward)   f32 mfma<144> 1.03   f32 mfma runtime act 1.64 (n = 96, elu, T = 8)
    f32 generic 3.19 (n = 144, elu / sigmoid, T = 9; 0.97 forced at n = 144 with tanh / sigmoid)   gemm+f32 scan 0.86
and the largest yardsticks: y32 2.09e-6 (linear / sigmoid, n = 128, T = 15), y22 of the layers on the scan plan 5.44e-7.  One finding
went into the yardstick, not the bound: rg.F32_ORDERS (gru_generic_kernel at n = 144, elu, T = 4: 4.03 times the BLAS-order y32)."""
import functools

import numpy as np
import pytest

from tests import ref_gru_forward as rg
from tests.gpu_util import Out, dev, nan_filled, need_gpu, padded_input as _padded_input, stream

pytestmark = pytest.mark.gpu

SHARE_CU = 1 << 10                             # include/sloika_amd.h: bit 10 of `reverse`
DIRECTIONS = [False, True]


@functools.lru_cache(maxsize=None)
def _weights(I, n, regime):
    return tuple(dev(a) for a in rg.weights(I, n, regime))


@functools.lru_cache(maxsize=None)
def _ring_is_two_groups(plan):
    gs, two = rg.declared_geometry(plan)
    return two and gs == {1: 4, 2: 4, 3: 2}[plan]


def _lib():
    need_gpu()
    from sloika_amd import _lib
    return _lib.lib()


def run_layer(c, plan, save=False, tell=True, flags=0, ldy=None, lead=0):
    """One slk_gru_bar16_f32 launch of case c -> (y, zr or None) as fetched Out objects, everything outside the outputs verified."""
    import torch
    L = _lib()
    assert plan == 0 or _ring_is_two_groups(plan)                      # 2 * GS == R for the plan under test
    I, n, T, B = c["I"], c["n"], c["T"], c["B"]
    lens = c["lens"]
    xd = _padded_input(c["x"], lens, I + 4)
    x0 = xd.clone()
    iW, sW, sW2, b = _weights(I, n, c["regime"])
    ld = None if lens is None or not tell else dev(np.asarray(lens, np.int32))
    y = Out(T, B, n, ldy, lead)
    zr = Out(T, B, 2 * n) if save else None
    rc = L.slk_gru_bar16_f32(xd.data_ptr(), I + 4, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.ptr(), y.ld, T, B, I, n,
                             int(c["reverse"]) | (plan << 8) | flags, 1, 2, None if ld is None else ld.data_ptr(),
                             None if zr is None else zr.ptr(), stream())
    what = "(%d,%d) plan %d T=%d B=%d" % (I, n, plan, T, B)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), x0.view(torch.int32)), what + ": x changed"
    y.fetch().assert_untouched_outside(lens if tell else None, what + " y")
    if zr is not None:
        zr.fetch().assert_untouched_outside(lens if tell else None, what + " zr")
    return y, zr


def _label(c, kernel, extra=""):
    return "%s (%d,%d) %s T=%d B=%d rev=%d lens=%d%s" % (kernel, c["I"], c["n"], c["regime"], c["T"], c["B"], int(bool(c["reverse"])),
                                                        c["lens"] is not None, extra)


def run_and_check(c, plan, save=False, **kw):
    y, zr = run_layer(c, plan, save, **kw)
    rg.check(y.values(), None if zr is None else zr.values(), c, _label(c, rg.KERNEL[plan], " save" if save else ""), rg.KERNEL[plan])
    return y, zr


# ------------------------------------------------------------------------------------------------------- time edges
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_time_edges(I, n, reverse):
    """T in rg.EDGE_T (moderate), the admitted lengths of `trained` and of the mixed-magnitude x, B = 17: full workgroups of every plan
    and a last one with a single live chunk and dead slots."""
    for regime, T, mixed in rg.edge_entries(I, n):
        c = rg.layer_case(I, n, regime, T, rg.EDGE_B, reverse, None, mixed)
        for plan in (1, 2, 3):
            run_and_check(c, plan)


# ------------------------------------------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_batch_edges(I, n, reverse):
    """T = 9, every B of rg.BATCH_B: the first B chunks of one case of 33 (chunks do not see each other)."""
    base = rg.layer_case(I, n, "moderate", rg.BATCH_T, max(rg.BATCH_B), reverse)
    for B in rg.BATCH_B:
        for plan in (1, 2, 3):
            run_and_check(base.take(B), plan)


@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_plan_by_batch_size(I, n):
    """Plan bits 0 at the first B whose four-chunk workgroups outnumber the CUs: the entry takes the eight-chunk kernel by itself
    (csrc/gru_bar16.hip: bar16_auto_plan), and the result has the bits of the forced eight-chunk plan.  T = 2 keeps it small."""
    torch = need_gpu()
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    B = 4 * ncu + 1
    assert (B + 3) // 4 > ncu >= (B + 7) // 8
    for reverse in DIRECTIONS:
        c = rg.layer_case(I, n, "moderate", rg.AUTO_T, B, reverse)
        assert max(c["yard"].values()) <= rg.ADMIT, c["yard"]
        y0, _ = run_layer(c, 0)
        rg.check(y0.values(), None, c, _label(c, "eight", " plan=auto"), "eight")
        y2, _ = run_and_check(c, 2)
        assert np.array_equal(y0.host, y2.host)
        run_and_check(c, 1)


# ----------------------------------------------------------------------------------------------------------- ragged
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_ragged(I, n, reverse):
    """T = 17, B = 33, lengths of rg.ragged_lens() told to the kernel: each chunk against float64 on the chunk alone, a reversed scan
    from the chunk's own last row.  Then T = 9 with every length equal to T: the bits of the call with lens = NULL."""
    c = rg.layer_case(I, n, "moderate", rg.RAGGED_T, rg.RAGGED_B, reverse, rg.ragged_lens())
    full = rg.layer_case(I, n, "moderate", rg.BATCH_T, rg.RAGGED_B, reverse, (rg.BATCH_T,) * rg.RAGGED_B)
    for plan in (1, 2, 3):
        run_and_check(c, plan)
        told, _ = run_and_check(full, plan)
        untold, _ = run_layer(full, plan, tell=False)
        assert np.array_equal(told.host, untold.host), (plan, "lens = T everywhere differs from lens = NULL")


# ------------------------------------------------------------------------------------------------------ saved gates
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_saved_gates(I, n, reverse):
    """zr_out at T in {1, 5, 9} and on the ragged case: z | r against float64, h the bits of the launch without zr_out."""
    cases = [rg.layer_case(I, n, "moderate", T, rg.EDGE_B, reverse) for T in rg.SAVE_T]
    cases.append(rg.layer_case(I, n, "moderate", rg.RAGGED_T, rg.RAGGED_B, reverse, rg.ragged_lens()))
    for c in cases:
        for plan in (1, 2, 3):
            plain, _ = run_layer(c, plan)
            saved, _ = run_and_check(c, plan, save=True)
            assert np.array_equal(plain.host, saved.host), (plan, c["T"], "h differs with zr_out")


# ------------------------------------------------------------------------------------------------- output placement
@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_output_placement(I, n):
    """y one float past a 16-byte boundary with ldy = n + 3.  The sixteen-chunk kernel stores 16 bytes at a time and the eight-chunk
    kernel 8: slk_gru_bar16q_launch and slk_gru_bar16d_launch both answer SLK_ERR_UNSUPPORTED here, so plans 2 and 3 fall through to
    the FOUR-chunk kernel (gru_bar16_kernel, 4-byte stores), which is the kernel this case checks under all three plan bits.  y two
    floats past the boundary with ldy = n + 2 suits 8-byte stores: there plan 3 falls to the eight-chunk kernel (gru_bar16d_kernel)
    and must give the bits plan 2 gives."""
    for reverse in DIRECTIONS:
        for c in (rg.layer_case(I, n, "moderate", rg.BATCH_T, rg.EDGE_B, reverse),
                  rg.layer_case(I, n, "moderate", rg.RAGGED_T, rg.RAGGED_B, reverse, rg.ragged_lens())):
            odd = {}
            for plan in (1, 2, 3):
                y, _ = run_layer(c, plan, ldy=n + 3, lead=1)
                rg.check(y.values(), None, c, _label(c, "four", " plan=%d ldy=n+3" % plan), "four")
                odd[plan] = y.host
            assert np.array_equal(odd[1], odd[2]) and np.array_equal(odd[1], odd[3])
            even = {}
            for plan in (2, 3):
                y, _ = run_layer(c, plan, ldy=n + 2, lead=2)
                rg.check(y.values(), None, c, _label(c, "eight", " plan=%d ldy=n+2" % plan), "eight")
                even[plan] = y.host
            assert np.array_equal(even[2], even[3])


# ------------------------------------------------------------------------------------------------------- CU sharing
@pytest.mark.parametrize("I,n", rg.SHARE_SHAPES + [(96, 96)])
def test_cu_sharing_bit(I, n):
    """Bit 10 of `reverse` with the four-chunk plan: layers up to 64 wide run without the exclusive LDS request (two workgroups may share
    a CU); above 64 wide the bit is ignored.  Either way: the bits of the same call without it."""
    for reverse in DIRECTIONS:
        for lens in (None, rg.share_lens()):
            c = rg.layer_case(I, n, "moderate", rg.BATCH_T, rg.SHARE_B, reverse, lens)
            for save in (False, True):
                y, zr = run_and_check(c, 1, save=save)
                ys, zrs = run_layer(c, 1, save=save, flags=SHARE_CU)
                rg.check(ys.values(), None if zrs is None else zrs.values(), c, _label(c, "four", " shared" + (" save" if save else "")), "four")
                assert np.array_equal(y.host, ys.host), (reverse, lens is not None, save)
                if save:
                    assert np.array_equal(zr.host, zrs.host), (reverse, lens is not None)


# ------------------------------------------------------------------------------------------------------------ stack
@pytest.mark.parametrize("nlayer", rg.STACK_LAYERS)
@pytest.mark.parametrize("n", rg.STACK_SIZES)
def test_stack_against_float64(n, nlayer):
    """slk_gru_bar16_stack_f32, (T, B) = (9, 5), directions alternating and starting reversed, the lengths told to the reversed layers only
    (what sloika_amd.layers does).  The buffers between the layers start as NaN: a reversed layer leaves the rows past a chunk's end as
    they are, the forward layer behind it (told no lengths) reads them and writes NaN there, and the next reversed layer must not read
    them.  The last layer's output over each chunk's own rows: finite and within BOUND of the float64 stack, the yardstick being
    the y22 stack, the cap 2e-5 per layer."""
    import torch
    from sloika_amd import _lib
    L = _lib.lib()
    need_gpu()
    assert _ring_is_two_groups(1)
    c = rg.stack_case(n, nlayer)
    T, B, lens = c["T"], c["B"], c["lens"]
    packs = []
    for iW, sW, sW2, b in c["layers"]:
        pk = torch.empty(L.slk_gru_bar16_pack_bytes(n, n), dtype=torch.uint8, device="cuda")
        assert pk.numel() > 0
        d = [dev(a) for a in (iW, b, sW, sW2)]
        assert L.slk_gru_bar16_pack_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, n, pk.data_ptr(), stream()) == 0
        packs.append(pk)
    xd = _padded_input(c["x"], lens, n + 4)
    x0 = xd.clone()
    ld = dev(np.asarray(lens, np.int32))
    y, tmp = Out(T, B, n), [Out(T, B, n), Out(T, B, n)]
    descs = (_lib.GruStackLayer * nlayer)()
    cur, ldcur = xd.data_ptr(), n + 4
    for k in range(nlayer):
        rev = (k + 1) & 1
        dst = y if k == nlayer - 1 else tmp[k & 1]
        descs[k] = _lib.GruStackLayer(cur, ldcur, dst.ptr(), n, packs[k].data_ptr(), rev | (0 if rev else _lib.SLK_GRU_STACK_NO_LENS), 0)
        cur, ldcur = dst.ptr(), n
    assert L.slk_gru_bar16_stack_f32(nlayer, descs, n, n, T, B, ld.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), x0.view(torch.int32))
    last_reversed = bool(nlayer & 1)
    y.fetch().assert_untouched_outside(lens if last_reversed else None, "stack output")
    for t in tmp:
        t.fetch().assert_untouched_outside(None, "stack buffer")
    if nlayer > 1:                                                    # the NaN rows were there for the reversed layers to avoid
        first = tmp[0].values()
        past = np.arange(T)[:, None] >= lens[None, :]
        assert np.isnan(first[past]).all()
    got = y.values()
    for b in range(B):
        assert np.isfinite(got[:lens[b], b]).all(), "chunk %d" % b
    rg.check(got, None, c, "stack (%d,%d) layers=%d T=%d B=%d" % (n, n, nlayer, T, B), "stack")


# -------------------------------------------------------------------------------------------------------- wide scan
def run_scan(c):
    import torch
    L = _lib()
    n, T, B, lens = c["n"], c["T"], c["B"], c["lens"]
    vd = _padded_input(c["vI"], lens, 3 * n + 8)
    v0 = vd.clone()
    _, sW, sW2, _ = _weights(c["I"], n, "moderate")
    ld = None if lens is None else dev(np.asarray(lens, np.int32))
    y = Out(T, B, n)
    rc = L.slk_gru_scan16_f32(vd.data_ptr(), 3 * n + 8, sW.data_ptr(), sW2.data_ptr(), y.ptr(), n, T, B, n, int(c["reverse"]), 1, 2,
                              None if ld is None else ld.data_ptr(), stream())
    assert rc == 0, (n, T, B, rc)
    torch.cuda.synchronize()
    assert torch.equal(vd.view(torch.int32), v0.view(torch.int32))
    y.fetch().assert_untouched_outside(lens, "scan y")
    rg.check(y.values(), None, c, _label(c, "scan1t"), "scan1t")


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rg.SCAN_SIZES)
def test_wide_scan(n, reverse):
    """slk_gru_scan16_f32 (csrc/gru_scan1t.hip): vI is the float32 rounding of the float64 projection, rows ldv = 3n + 8 apart with NaN
    in the gaps and in the rows past a chunk's end.  Step s takes its vI from register set s % 4 and requests step s + 3
    (gru_scan1t.hip:137-143, :171; the step loop is unrolled by four, :243-248): T in 1 .. 9 and both sides of 12 | 13 and 16 | 17 at
    B = 17, and the ragged case."""
    assert rg.declared_scan_period() == (4, 3)
    for T in rg.SCAN_T:
        run_scan(rg.scan_case(n, T, rg.EDGE_B, reverse))
    run_scan(rg.scan_case(n, rg.RAGGED_T, rg.RAGGED_B, reverse, rg.ragged_lens()))


# ------------------------------------------------------------------------------- the float32 scan (csrc/recurrent.hip)
F32_GEOMETRY = {"KB": (128, 8, 4), "tile": 4}
ALIGNED = dict(extra=0, lead=0)                # rows n apart from a 16-byte boundary: flush_block stores 16 bytes at a time
ODD = dict(extra=3, lead=1)                    # rows n + 3 apart, the first one float past a 16-byte boundary: its scalar stores
STORES = [ALIGNED, ODD]
STORE_IDS = ["vector", "scalar"]
PLAIN = ("tanh", "sigmoid")


@functools.lru_cache(maxsize=None)
def _f32_geometry_is_as_declared():
    return rg.declared_f32_scan_geometry() == F32_GEOMETRY


@functools.lru_cache(maxsize=None)
def _f32_weights(n):
    """(sW, sW2) of rg.f32_scan_case on the device, and copies to compare them with after a launch."""
    c = rg.f32_scan_case(n, 1, 1, False)
    sW, sW2 = dev(c["sW"]), dev(c["sW2"])
    return sW, sW2, sW.clone(), sW2.clone()


def f32_kernel(c, force_generic=0):
    """The kernel of csrc/recurrent.hip a case lands on (gru_recurrent_entry, launch_gru_mfma, launch_gru_mfma144)."""
    n, plain = c["n"], (c["act"], c["gate"]) == PLAIN
    if force_generic or n not in rg.F32_MFMA_SIZES or (n == 144 and not plain):
        return "f32 generic"
    if not plain:
        return "f32 mfma runtime act"
    return "f32 mfma<144>" if n == 144 else "f32 mfma<4 waves>"


def _f32_label(c, kernel, note=""):
    return "%s n=%d %s/%s T=%d B=%d rev=%d lens=%d%s" % (kernel, c["n"], c["act"], c["gate"], c["T"], c["B"], int(bool(c["reverse"])),
                                                        c["lens"] is not None, note)


def run_f32(c, entry=None, extra=0, lead=0, force_generic=0):
    """One launch of case c -> y as a fetched Out, everything outside the output verified.  entry None: slk_gru_recurrent_f32, or
    slk_gru_recurrent_ragged_f32 where the case has lengths; "ragged": the ragged entry, with every length T where the case has none;
    "ex": slk_gru_recurrent_f32_ex with force_generic.  vI is dense (the entries take no ldv) from a 16-byte boundary, with NaN in
    every row at t >= lens[b]."""
    import torch
    L = _lib()
    assert _f32_geometry_is_as_declared(), rg.declared_f32_scan_geometry()
    n, T, B, lens = c["n"], c["T"], c["B"], c["lens"]
    vd = _padded_input(c["vI"], lens, 3 * n)
    assert vd.data_ptr() % 16 == 0 and vd.is_contiguous()
    v0 = vd.clone()
    sW, sW2, sW_0, sW2_0 = _f32_weights(n)
    act, gate = rg.ACTIVATIONS[c["act"]][1], rg.ACTIVATIONS[c["gate"]][1]
    y = Out(T, B, n, n + extra, lead)
    args = (vd.data_ptr(), sW.data_ptr(), sW2.data_ptr(), y.ptr(), y.ld, T, B, n, int(c["reverse"]), act, gate)
    if entry == "ex" or force_generic:
        assert lens is None
        rc = L.slk_gru_recurrent_f32_ex(*args, force_generic, stream())
    elif lens is not None or entry == "ragged":
        ld = dev(np.asarray(lens, np.int32) if lens is not None else np.full(B, T, np.int32))
        rc = L.slk_gru_recurrent_ragged_f32(*args, ld.data_ptr(), stream())
    else:
        rc = L.slk_gru_recurrent_f32(*args, stream())
    what = _f32_label(c, f32_kernel(c, force_generic))
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    for now, before in ((vd, v0), (sW, sW_0), (sW2, sW2_0)):
        assert torch.equal(now.view(torch.int32), before.view(torch.int32)), what + ": an input changed"
    y.fetch().assert_untouched_outside(lens, what)
    return y


def f32_twice(c, note="", **kw):
    """The case twice: within the bound of its y32 yardstick, and the second launch with the bits of the first."""
    kernel = f32_kernel(c, kw.get("force_generic", 0))
    note += " ldh=n+%d lead=%d" % (kw.get("extra", 0), kw.get("lead", 0))
    y = run_f32(c, **kw)
    rg.check(y.values(), None, c, _f32_label(c, kernel, note), kernel)
    assert np.array_equal(y.host, run_f32(c, **kw).host), _f32_label(c, kernel, note + ": the second launch differs")
    return y


@pytest.mark.parametrize("store", STORES, ids=STORE_IDS)
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rg.F32_MFMA_SIZES)
def test_f32_mfma_time_edges(n, reverse, store):
    """gru_mfma_kernel through slk_gru_recurrent_f32: every T of the size's rg.F32_T (both slots of the DMA ring, the first refill of
    either, the request that would pass the end, the late and the tail flush) at B = 17, in both store paths."""
    for T in rg.F32_T[rg.f32_kb(n)]:
        c = rg.f32_scan_case(n, T, rg.F32_EDGE_B, reverse)
        assert f32_kernel(c).startswith("f32 mfma<")
        f32_twice(c, **store)


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rg.F32_MFMA_SIZES)
def test_f32_mfma_batch_edges(n, reverse):
    """T = KB + 1, every B of rg.F32_BATCH_B: the first B chunks of one case of nine (chunks do not see each other); a last tile of
    one, two and three live chunks, whose dead slots re-read chunk B - 1."""
    base = rg.f32_scan_case(n, rg.f32_kb(n) + 1, max(rg.F32_BATCH_B), reverse)
    for B in rg.F32_BATCH_B:
        f32_twice(base.take(B), **(ODD if B % 2 else ALIGNED))


@pytest.mark.parametrize("store", STORES, ids=STORE_IDS)
@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rg.F32_MFMA_SIZES)
def test_f32_mfma_ragged(n, reverse, store):
    """slk_gru_recurrent_ragged_f32 on the lengths of rg.f32_ragged_lens (tiles of four different lengths, one of ones, a last chunk
    of one step): each chunk against float64 on the chunk alone, a reversed scan from the chunk's own last row.  Then every length
    equal to T: the bits of slk_gru_recurrent_f32."""
    T, lens = rg.f32_ragged_lens(rg.f32_kb(n))
    f32_twice(rg.f32_scan_case(n, T, rg.F32_RAGGED_B, reverse, lens), **store)
    full = rg.f32_scan_case(n, T, rg.F32_RAGGED_B, reverse, (T,) * rg.F32_RAGGED_B)
    told = f32_twice(full, **store)
    plain = rg.Case(**dict(full, lens=None))                           # the same inputs, no lengths told
    assert np.array_equal(told.host, run_f32(plain, **store).host), "lens = T everywhere differs from slk_gru_recurrent_f32"


@pytest.mark.parametrize("act,gate", rg.OTHER_PAIRS)
@pytest.mark.parametrize("n", rg.F32_ACT_SIZES + (144,))
def test_f32_runtime_activations(n, act, gate):
    """Other activations: gru_mfma_kernel<N, -1, -1> at n up to 128, and at n = 144, where only tanh / sigmoid fits the twelve-wave form
    (launch_gru_mfma144), the portable kernel -- which must still be within the bound.  T in (1, KB, KB + 1, 2 KB + 1) forward, B = 5,
    and one ragged reversed case."""
    want = "f32 generic" if n == 144 else "f32 mfma runtime act"
    for k, T in enumerate(rg.F32_ACT_T[(n, act)]):
        c = rg.f32_scan_case(n, T, rg.F32_ACT_B, False, None, act, gate)
        assert f32_kernel(c) == want
        f32_twice(c, **STORES[k & 1])
    f32_twice(rg.f32_scan_case(n, max(rg.F32_ACT_LENS), rg.F32_ACT_B, True, rg.F32_ACT_LENS, act, gate), **ODD)


@pytest.mark.parametrize("n", rg.F32_GENERIC_SIZES + rg.F32_FORCED_SIZES)
def test_f32_generic_kernel(n):
    """gru_generic_kernel.  Sizes without an MFMA instantiation through both entries: T in (1, 2, 9), B in (1, 5), and the lengths
    (9, 1, 4, 5, 8), both directions, rows n + 3 apart off alignment.  Sizes that have one, with force_generic = 1 of
    slk_gru_recurrent_f32_ex: the size's time-edge cases at T in (1, KB + 1), B = 17."""
    if n in rg.F32_FORCED_SIZES:
        for reverse in DIRECTIONS:
            for T in (1, rg.f32_kb(n) + 1):
                c = rg.f32_scan_case(n, T, rg.F32_EDGE_B, reverse)
                forced = f32_twice(c, " forced", force_generic=1, **ODD)
                assert f32_kernel(c, 1) == "f32 generic" and f32_kernel(c) != "f32 generic"
                assert forced.values().shape == (T, rg.F32_EDGE_B, n)
        return
    for reverse in DIRECTIONS:
        for T in rg.F32_GENERIC_T:
            base = rg.f32_scan_case(n, T, max(rg.F32_GENERIC_B), reverse)
            assert f32_kernel(base) == "f32 generic"
            for B in rg.F32_GENERIC_B:
                plain = f32_twice(base.take(B), **ODD)
                told = f32_twice(base.take(B), " ragged entry", entry="ragged", **ODD)
                assert np.array_equal(plain.host, told.host)
        f32_twice(rg.f32_scan_case(n, max(rg.F32_GENERIC_LENS), max(rg.F32_GENERIC_B), reverse, rg.F32_GENERIC_LENS), **ODD)


@pytest.mark.parametrize("reverse", DIRECTIONS)
@pytest.mark.parametrize("n", rg.F32_LONG_SIZES)
def test_f32_long(n, reverse):
    """T = 100, B = 6: a dozen turnovers of both rings on four waves (n = 96) and twenty-five on twelve (n = 144)."""
    f32_twice(rg.f32_scan_case(n, rg.F32_LONG_T[n], rg.F32_LONG_B, reverse), **ALIGNED)


@pytest.mark.parametrize("I,n", rg.F32_LAYER_SHAPES)
def test_f32_layer_fallback(I, n):
    """slk_gru_f32 where no whole-layer kernel takes the shape: projection GEMM into the workspace + the float32 scan, x rows I + 4
    apart and y rows n + 3 apart off alignment, against float64 from x; the yardstick is y32 of the whole layer, projection included.
    A missing workspace or one a byte short: SLK_ERR_WORKSPACE, and neither y nor the workspace is written."""
    import torch
    from sloika_amd import _lib as lib_module
    L = _lib()
    T, B = rg.F32_LAYER_TB
    need = L.slk_gru_workspace_bytes(T, B, n)
    assert need == 4 * T * B * 3 * n
    z = dev(np.zeros(4, np.float32))
    assert L.slk_gru_bar16_f32(z.data_ptr(), I, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, z.data_ptr(), n, 1, 1, I, n, 0, 1, 2,
                               None, None, stream()) == lib_module.SLK_ERR_UNSUPPORTED   # no whole-layer kernel: the fallback runs
    iW, sW, sW2, b = _weights(I, n, "moderate")
    for reverse in DIRECTIONS:
        c = rg.f32_layer_case(I, n, T, B, reverse)
        xd = _padded_input(c["x"], None, I + 4)
        x0 = xd.clone()
        ws = dev(nan_filled(need // 4 + 64))
        w0 = ws.clone()
        assert ws.data_ptr() % 16 == 0
        y = Out(T, B, n, n + 3, 1)
        args = (xd.data_ptr(), I + 4, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.ptr(), y.ld, T, B, I, n, int(reverse), 1, 2)
        assert L.slk_gru_f32(*args, ws.data_ptr(), need - 1, stream()) == lib_module.SLK_ERR_WORKSPACE
        assert L.slk_gru_f32(*args, None, need, stream()) == lib_module.SLK_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.equal(ws.view(torch.int32), w0.view(torch.int32)), "a refused call wrote the workspace"
        assert (y.fetch().host == y.host[0]).all(), "a refused call wrote y"
        what = "gemm+f32 scan (%d,%d) T=%d B=%d rev=%d" % (I, n, T, B, reverse)
        results = []
        for _ in range(2):
            assert L.slk_gru_f32(*args, ws.data_ptr(), need, stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(xd.view(torch.int32), x0.view(torch.int32)), what + ": x changed"
            assert torch.equal(ws[need // 4:].view(torch.int32), w0[need // 4:].view(torch.int32)), "written past the workspace"
            y.fetch().assert_untouched_outside(None, what)
            results.append(y.host)
        rg.check(y.values(), None, c, what, "gemm+f32 scan")
        assert np.array_equal(results[0], results[1]), what + ": the second launch differs"


def _net_case(I, n, act, gate, grade, reverse):
    T, lens = rg.f32_ragged_lens(8)
    return rg.f32_layer_case(I, n, T, rg.F32_RAGGED_B, reverse, lens, grade, act, gate)


def _run_birnn(I, n, act, gate, grade):
    """layers.birnn of two Gru(I, n) with the weights of rg.weights under layers.ragged(lens): each direction's half of the output
    against the float64 recursion of every chunk alone, over that chunk's own steps."""
    import torch
    from sloika_amd import activation, layers
    fun, gatefun = getattr(activation, act), getattr(activation, gate)
    assert layers.gru_plan(I, n, fun, gatefun) == "scan" and layers.gru_pad_shape(I, n, fun, gatefun) == (I, n)
    iW, sW, sW2, b = rg.weights(I, n, "moderate")
    grus = []
    for _ in range(2):
        g = layers.Gru(I, n, has_bias=True, fun=fun, gatefun=gatefun)
        g.set_params({"iW": iW.reshape(3, n, I), "sW": sW.reshape(2, n, n), "sW2": sW2, "b": b.reshape(3, n)})
        grus.append(g)
    net = layers.birnn(grus[0], grus[1])
    fwd, bwd = (_net_case(I, n, act, gate, grade, reverse) for reverse in DIRECTIONS)
    T, B, lens = fwd["T"], fwd["B"], fwd["lens"]
    assert np.array_equal(fwd["x"], bwd["x"])
    xd = _padded_input(fwd["x"], lens, I)                               # NaN behind every chunk's end
    x0 = xd.clone()
    runs = []
    for _ in range(2):
        with layers.ragged(lens):
            runs.append(net.run(xd).cpu().numpy())
        torch.cuda.synchronize()
        assert torch.equal(xd.view(torch.int32), x0.view(torch.int32))
    assert runs[0].shape == (T, B, 2 * n)
    own = np.arange(T)[:, None] < lens[None, :]
    assert np.array_equal(runs[0][own].view(np.uint32), runs[1][own].view(np.uint32)), "the second run differs"
    kernel = f32_kernel(fwd) if grade == "y22" else "gemm+f32 scan"
    for c, half in ((fwd, runs[0][:, :, :n]), (bwd, runs[0][:, :, n:])):
        rg.check(half, None, c, "layers.Gru(%d,%d) %s/%s %s rev=%d" % (I, n, act, gate, kernel, c["reverse"]), kernel)


@pytest.mark.parametrize("I,n,act,gate", rg.F32_NET_SCAN)
def test_f32_scan_is_what_the_layer_runs(I, n, act, gate):
    """layers.Gru on the "scan" plan (wider than 144; other activations), ragged inside a birnn: the forward half through
    slk_gru_recurrent_f32, the reversed half through slk_gru_recurrent_ragged_f32.  The projection is the fp16 split: yardstick y22 of
    the whole layer."""
    need_gpu()
    _run_birnn(I, n, act, gate, "y22")


def test_f32_scan_is_what_the_layer_runs_in_exact_f32_mode(monkeypatch):
    """layers.SPLIT_F16 = False (SLOIKA_AMD_EXACT_F32=1): a fresh Gru(96, 96) leaves the whole-layer kernel for the float32 GEMM and
    the float32 scan: yardstick y32 of the whole layer."""
    need_gpu()
    from sloika_amd import activation, layers
    I, n = rg.F32_NET_EXACT
    assert layers.gru_plan(I, n, activation.tanh, activation.sigmoid) == "layer"
    monkeypatch.setattr(layers, "SPLIT_F16", False)
    _run_birnn(I, n, "tanh", "sigmoid", "y32")


# ---------------------------------------------------------------------------------------------------------- figures
def test_recorded_figures():
    """The worst err / yardstick per kernel and the largest yardstick per grade and regime over the GRUFWD lines of this run
    (design/gru.md keeps the table of the whole-layer kernels, the module docstring that of the float32 scan).  A ratio above BOUND[0]
    has already failed its own test; here it fails once more, by name."""
    for kernel, ratio in sorted(rg.FIGURES["ratio"].items()):
        print("GRUFWD-SUMMARY kernel %s worst ratio %.2f" % (kernel, ratio))
    for grade in ("y22", "y32"):
        for regime, y in sorted(rg.FIGURES[grade].items()):
            print("GRUFWD-SUMMARY regime %s largest %s %.3e" % (regime, grade, y))
    assert all(r <= rg.BOUND[0] for r in rg.FIGURES["ratio"].values()), rg.FIGURES["ratio"]
    assert all(y <= rg.ADMIT for grade in ("y22", "y32") for y in rg.FIGURES[grade].values()), rg.FIGURES
