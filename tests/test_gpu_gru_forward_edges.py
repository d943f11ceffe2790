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

References and yardsticks are made once per (shape, regime, T, direction) and shared by the plans and the tests (rg.layer_case)."""
import functools

import numpy as np
import pytest

from tests import ref_gru_forward as rg
from tests.gpu_util import Out, dev, need_gpu, padded_input as _padded_input, stream

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


# ---------------------------------------------------------------------------------------------------------- figures
def test_recorded_figures():
    """The worst err / yardstick per kernel and the largest y22 per regime over the GRUFWD lines of this run (design/gru.md keeps
    the table).  A ratio above BOUND[0] has already failed its own test; here it fails once more, by name."""
    for kernel, ratio in sorted(rg.FIGURES["ratio"].items()):
        print("GRUFWD-SUMMARY kernel %s worst ratio %.2f" % (kernel, ratio))
    for regime, y in sorted(rg.FIGURES["y22"].items()):
        print("GRUFWD-SUMMARY regime %s largest y22 %.3e" % (regime, y))
    assert all(r <= rg.BOUND[0] for r in rg.FIGURES["ratio"].values()), rg.FIGURES["ratio"]
    assert all(y <= rg.ADMIT for y in rg.FIGURES["y22"].values()), rg.FIGURES["y22"]
