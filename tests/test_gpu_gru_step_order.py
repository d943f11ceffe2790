"""Where in a step the chain waves of the four-chunk Gru kernel (csrc/gru_bar16_body.h) store h(s-1) and z, ask for vI(s), and form
sigmoid(z), 1 - z and z*h is a schedule (design/gru_step_order.md): the store of h(s-1) happens a step late, out of `hold`, behind
the first products of step s; the update gate's epilogue is spread among the candidate's products.  What such a move can break, and
what the recorded bits of the other tests only graze:

  * a store that takes `hold` after the step overwrote it, that writes a row past its chunk's end, or that is skipped where the four
    chunks of a workgroup end in four different steps of a group of four;
  * a blend that takes the z*h or the 1 - z of the step before.

The four-chunk launches are compared bit for bit with the eight-chunk plan (csrc/gru_bar16d.hip, another kernel with another
schedule, forced through bits 8-9 of `reverse`) and with tests/ref_gru_forward.py's float64 recursion under that file's own bound.
Outputs are pre-filled with a canary: rows past a chunk's end must still hold it."""
import functools

import numpy as np
import pytest

from tests import ref_gru_forward as R

pytestmark = pytest.mark.gpu

N = 96
TS = (1, 2, 3, 4, 5, 8, 9)
BS = (1, 4, 5, 9)
BMAX = max(BS)
PLAN_FOUR, PLAN_EIGHT = 1 << 8, 2 << 8
CANARY = np.float32(-5.0)                       # |h| < 1 and 0 < z, r < 1: no kernel computes it


def phase_lens(T):
    """Workgroup 0 (chunks 0-3): the four chunks end in four different steps of a group of four, T, T-1, T-2, T-3 floored at 1.
    Workgroup 1 (chunks 4-7) holds a chunk of length 1 next to full ones; chunk 8 is alone in its workgroup."""
    return tuple(max(1, v) for v in (T, T - 1, T - 2, T - 3, 1, T, T // 2, T, T - 1))


@functools.lru_cache(maxsize=None)
def layer_case(T, reverse, lens_on):
    iW, sW, sW2, b = R.weights(N, N, "moderate")
    x = R.inputs(N, T, BMAX, 900 + T)
    ln = np.asarray(phase_lens(T), np.int32) if lens_on else None
    h, zr = R.gru_forward(x, iW, sW, sW2, b, reverse, ln)
    h22, zr22 = R.gru_forward(x, iW, sW, sW2, b, reverse, ln, R.F32, 22)
    return R.Case(I=N, n=N, regime="moderate", T=T, B=BMAX, reverse=reverse, lens=ln, x=x, vI=None, iW=iW, sW=sW, sW2=sW2, b=b,
                  h=h, zr=zr, h22=h22, zr22=zr22, cap=R.CAP)


def stack_forward(x, layers, first, lens, dtype=R.F64, bits=None):
    """Layers of alternating direction, layer 0 reversed iff `first`: every layer's h."""
    outs, cur = [], x
    for k, (iW, sW, sW2, b) in enumerate(layers):
        cur = R.gru_forward(cur, iW, sW, sW2, b, bool((k + first) & 1), lens, dtype, bits)[0]
        if lens is not None:                    # what the next layer reads past a chunk's end is never used: any finite value
            cur = np.where(np.isnan(cur), dtype(0), cur)
        outs.append(cur)
    return outs


@functools.lru_cache(maxsize=None)
def stack_case(nlayer, T, first, lens_on):
    layers = R.stack_weights(N, nlayer)
    x = R.inputs(N, T, BMAX, 1700 + T)
    ln = np.asarray(phase_lens(T), np.int32) if lens_on else None
    h = stack_forward(x, layers, first, ln)[-1]
    h22 = stack_forward(x, layers, first, ln, R.F32, 22)[-1]
    return R.Case(I=N, n=N, regime="moderate", T=T, B=BMAX, reverse=None, lens=ln, x=x, vI=None, layers=layers, h=h, zr=None, h22=h22,
                  zr22=None, cap=R.CAP * nlayer)


def same_bits(a, b, what):
    same = a.view(np.uint32) == b.view(np.uint32)
    assert same.all(), "%s differs at %s: %s against %s" % (what, np.argwhere(~same)[:4].tolist(), a[~same][:4], b[~same][:4])


def canary_kept(out, lens, what):
    """Rows at and past a chunk's end still hold the canary, every row of the chunk's own steps was written."""
    T, B = out.shape[:2]
    for b in range(B):
        end = T if lens is None else int(lens[b])
        assert (out[end:, b] == CANARY).all(), "%s: chunk %d (length %d) was written past its end" % (what, b, end)
        assert (out[:end, b] != CANARY).all(), "%s: chunk %d (length %d) keeps the canary inside its steps" % (what, b, end)


def launch(L, plan, xd, wd, T, B, reverse, ld, save):
    import torch
    from tests.gpu_util import stream
    y = torch.full((T, B, N), float(CANARY), dtype=torch.float32, device="cuda")
    zr = torch.full((T, B, 2 * N), float(CANARY), dtype=torch.float32, device="cuda") if save else None
    iW, sW, sW2, b = wd
    rc = L.slk_gru_bar16_f32(xd.data_ptr(), N, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.data_ptr(), N, T, B, N, N,
                             int(reverse) | plan, 1, 2, None if ld is None else ld.data_ptr(), None if zr is None else zr.data_ptr(), stream())
    assert rc == 0, rc
    return y.cpu().numpy(), None if zr is None else zr.cpu().numpy()


@pytest.mark.parametrize("reverse", [False, True])
def test_h_and_z_are_stored_once_per_step_at_every_phase(reverse):
    """96 -> 96 layer launch with and without saved gates."""
    from tests.gpu_util import dev, need_gpu
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    wd = tuple(dev(a) for a in R.weights(N, N, "moderate"))
    for T in TS:
        for lens_on in (True, False):
            full = layer_case(T, reverse, lens_on)
            for B in BS:
                case = full.take(B)
                xd = dev(case["x"])
                ld = None if case["lens"] is None else dev(case["lens"])
                what = "T=%d B=%d reverse=%d ragged=%d" % (T, B, reverse, lens_on)
                h4, _ = launch(L, PLAN_FOUR, xd, wd, T, B, reverse, ld, False)
                h4s, zr4 = launch(L, PLAN_FOUR, xd, wd, T, B, reverse, ld, True)
                h8, zr8 = launch(L, PLAN_EIGHT, xd, wd, T, B, reverse, ld, True)
                for out, nm in ((h4, "h"), (h4s, "h with saved gates"), (zr4, "z | r"), (h8, "h of the eight-chunk plan")):
                    canary_kept(out, case["lens"], what + " " + nm)
                same_bits(h4, h8, what + ": h, four chunks against eight")
                same_bits(h4s, h8, what + ": h with saved gates, four chunks against eight")
                same_bits(zr4, zr8, what + ": z | r, four chunks against eight")
                # (the reference marks rows past a chunk's end with NaN and compares a chunk's own steps only)
                R.check(h4, None, case, what + " plain")
                R.check(h4s, zr4, case, what + " saved gates")


@pytest.mark.parametrize("nlayer", [1, 3])
def test_packed_and_stacked_layers_store_every_step_at_every_phase(nlayer):
    """The packed stack of one layer and of three with alternating direction, starting in either direction."""
    from tests.gpu_util import dev, need_gpu, stream
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    layers = R.stack_weights(N, nlayer)
    ws, packs = [], []
    for iW, sW, sW2, b in layers:
        wd = tuple(dev(a) for a in (iW, sW, sW2, b))
        pk = torch.empty(L.slk_gru_bar16_pack_bytes(N, N), dtype=torch.uint8, device="cuda")
        assert pk.numel() > 0
        assert L.slk_gru_bar16_pack_f32(wd[0].data_ptr(), wd[3].data_ptr(), wd[1].data_ptr(), wd[2].data_ptr(), N, N, pk.data_ptr(), stream()) == 0
        ws.append(wd)
        packs.append(pk)
    for first in (1, 0):
        for T in TS:
            for lens_on in (True, False):
                full = stack_case(nlayer, T, first, lens_on)
                for B in BS:
                    case = full.take(B)
                    xd = dev(case["x"])
                    ld = None if case["lens"] is None else dev(case["lens"])
                    what = "%d layers, first reversed=%d, T=%d B=%d ragged=%d" % (nlayer, first, T, B, lens_on)
                    outs = [torch.full((T, B, N), float(CANARY), dtype=torch.float32, device="cuda") for _ in packs]
                    descs = (_lib.GruStackLayer * nlayer)()
                    cur = xd
                    for k, pk in enumerate(packs):
                        descs[k] = _lib.GruStackLayer(cur.data_ptr(), N, outs[k].data_ptr(), N, pk.data_ptr(),
                                                      ((k + first) & 1) | (_lib.SLK_GRU_STACK_NO_LENS if ld is None else 0), 0)
                        cur = outs[k]
                    rc = L.slk_gru_bar16_stack_f32(nlayer, descs, N, N, T, B, None if ld is None else ld.data_ptr(), stream())
                    assert rc == 0, rc
                    got = [o.cpu().numpy() for o in outs]
                    cur = xd
                    for k in range(nlayer):                           # the same layers, one eight-chunk launch each, same canary
                        canary_kept(got[k], case["lens"], what + " layer %d" % (k + 1))
                        want, _ = launch(L, PLAN_EIGHT, cur, (ws[k][0], ws[k][1], ws[k][2], ws[k][3]), T, B, (k + first) & 1, ld, False)
                        same_bits(got[k], want, what + ": layer %d, stack against eight-chunk launches" % (k + 1))
                        cur = dev(want)
                    R.check(got[-1], None, case, what)


# ------------------------------------------------------------------------------------------------------ a stale update gate
GATE_T, GATE_B = 5, 4
#: chunk c takes the candidate at step s where OPEN[c][s] (z = 0) and keeps its state elsewhere (z = 1).  Step 0 opens everywhere,
#: so every later step has a state to keep, and every chunk has both transitions.
OPEN = ((1, 0, 0, 0, 0), (1, 1, 0, 1, 0), (1, 0, 1, 0, 0), (1, 1, 1, 0, 0))


def gate_weights(zbias):
    """The moderate weights with the z rows of the bias at `zbias`; `zbias` None: at -30, and the z rows of iW take 60 x[0]."""
    iW, sW, sW2, b = (a.copy() for a in R.weights(N, N, "moderate"))
    if zbias is None:
        b[:N] = -30.0
        iW[:N] = 0.0
        iW[:N, 0] = 60.0
    else:
        b[:N] = zbias
    return iW, sW, sW2, b


def gate_input(reverse, switched):
    x = R.inputs(N, GATE_T, GATE_B, 77)
    if switched:                                # x[t][c][0] = 0 where the step at time t is open, 1 where it keeps
        for c in range(GATE_B):
            for s in range(GATE_T):
                x[GATE_T - 1 - s if reverse else s, c, 0] = 0.0 if OPEN[c][s] else 1.0
    return x


@pytest.mark.parametrize("reverse", [False, True])
def test_the_blend_takes_this_steps_update_gate(reverse):
    """|z's pre-activation| >= 30 - |h.sW_z| - |x.iW_z| > 17, so sigmoid(z) = 1 / (1 + 2^(-1.44 v)) is 1 exactly or below 2^-24: with z = 1
    the blend fmaf(1 - z, c, z h) returns h(s-1) bit for bit, with z = 0 the candidate (z h < 2^-24 |h| is under half an ulp of any
    candidate above 2^-24 |h|; the eight-chunk plan, which shares the arithmetic and not the schedule, says which bits that is)."""
    from tests.gpu_util import dev, need_gpu
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B = GATE_T, GATE_B
    for zbias, switched in ((30.0, False), (-30.0, False), (None, True)):
        w = gate_weights(zbias)
        x = gate_input(reverse, switched)
        wd, xd = tuple(dev(a) for a in w), dev(x)
        what = "z bias %s reverse=%d" % (zbias, reverse)
        h4, zr4 = launch(L, PLAN_FOUR, xd, wd, T, B, reverse, None, True)
        h4p, _ = launch(L, PLAN_FOUR, xd, wd, T, B, reverse, None, False)
        h8, zr8 = launch(L, PLAN_EIGHT, xd, wd, T, B, reverse, None, True)
        same_bits(h4, h8, what + ": h with saved gates, four chunks against eight")
        same_bits(h4p, h8, what + ": h, four chunks against eight")
        same_bits(zr4, zr8, what + ": z | r, four chunks against eight")
        ref, _ = R.gru_forward(x, *w, reverse)
        ref22, _ = R.gru_forward(x, *w, reverse, None, R.F32, 22)
        yard = float(np.abs(ref22 - ref).max())
        err = float(np.abs(h4p.astype(np.float64) - ref).max())
        print("GATE %s err %.3e yardstick %.3e" % (what, err, yard))
        assert err <= R.BOUND[0] * yard + R.BOUND[1] and err <= R.CAP, (what, err, yard)
        order = [T - 1 - s for s in range(T)] if reverse else list(range(T))        # time index of scan step s
        z = zr4[..., :N]
        for h in (h4, h4p):
            if zbias == 30.0:                   # the state never leaves h(-1) = 0
                assert (z == 1.0).all() and (h == 0.0).all(), what
            elif zbias == -30.0:
                assert (z < 2.0 ** -24).all(), what
            else:
                for c in range(B):
                    for s in range(T):
                        now = h[order[s], c]
                        if OPEN[c][s]:
                            assert (z[order[s], c] < 2.0 ** -24).all(), (what, c, s)
                            if s > 0:           # a candidate of its own, not the state kept
                                assert (now != h[order[s - 1], c]).any(), (what, c, s)
                        else:
                            assert (z[order[s], c] == 1.0).all(), (what, c, s)
                            same_bits(now, h[order[s - 1], c], what + ": chunk %d keeps its state at step %d" % (c, s))
