"""The projection tiles of the four-chunk Gru kernel (csrc/gru_bar16_body.h), one by one: which wave computes a tile of vI = iW.x + b, in
which interval of the step, and from which operand image in LDS it takes x, is a schedule (design/gru_projection.md) -- a tile taken from
the wrong image or ring slot, by the wrong wave, a group too early or too late, or from the layer before in a stack, is a wrong vI row
block and nothing else.

So the recurrent weights are ZERO here: h(s) = z h(s-1) + (1 - z) tanh(vc) with z = sigmoid(vz), and every one of the 3n/16 tiles of vI
decides sixteen outputs on its own -- the z and c tiles through h, the r tiles (which a zero sW2 hides from h) through the saved gates
of the training variant.  The rows of iW are random, so no two tiles agree.

  * against tests/ref_gru_forward.py's float64 recursion under that file's own bound (`check`);
  * bit for bit against the eight-chunk plan (bits 8-9 of `reverse`), whose projection is scheduled differently.

Shapes: the instantiations whose chain waves carry projection tiles behind their write of r*h (96 -> 96, 32 -> 96, 64 -> 96), at T in
{1, 3, 4, 5, 8, 9} (group 0 alone, a group not full, full, the first turnover of the operand images, the ring's), B in {1, 4, 5}, both
directions, full and ragged with a chunk of length 1.  Forms: the layer launch with and without saved gates, the packed layer (a stack
of one), and layers 2 and 3 of a stack of three whose layers have different iW (a stale image across the boundary is layer 1's tile).
Last, a repeat-launch screen with every CU busy.

Inputs are numpy integers scaled by powers of two: the same bits on every host."""
import functools

import numpy as np
import pytest

from tests import ref_gru_forward as R

pytestmark = pytest.mark.gpu

SHAPES = [(96, 96), (32, 96), (64, 96)]
TS = (1, 3, 4, 5, 8, 9)
BS = (1, 4, 5)
BMAX = max(BS)
PLAN_FOUR, PLAN_EIGHT = 1 << 8, 2 << 8
FILL = -5.0


def tile_weights(I, n, k=0):
    """|iW| < 1/8, |b| < 1, sW = sW2 = 0."""
    rs = np.random.RandomState(7000 + 13 * I + n + 101 * k)
    iW = (rs.randint(-4096, 4096, size=(3 * n, I)) / 32768.0).astype(np.float32)
    b = (rs.randint(-4096, 4096, size=3 * n) / 4096.0).astype(np.float32)
    return iW, np.zeros((2 * n, n), np.float32), np.zeros((n, n), np.float32), b


def tile_input(I):
    return (np.random.RandomState(50 + I).randint(-32768, 32768, size=(max(TS), BMAX, I)) / 16384.0).astype(np.float32)


def ragged(T):
    """Chunk 0 has length 1 (so the batch of one chunk has it too), the others both sides of a group of four where T allows."""
    return tuple(int(v) for v in (1, T, max(1, T - 1), max(1, T // 2), min(T, 5)))


@functools.lru_cache(maxsize=None)
def layer_case(I, n, T, reverse, lens_on):
    iW, sW, sW2, b = tile_weights(I, n)
    x = np.ascontiguousarray(tile_input(I)[:T])
    ln = np.asarray(ragged(T), np.int32) if lens_on else None
    h, zr = R.gru_forward(x, iW, sW, sW2, b, reverse, ln)
    h22, zr22 = R.gru_forward(x, iW, sW, sW2, b, reverse, ln, R.F32, 22)
    return R.Case(I=I, n=n, regime="moderate", T=T, B=BMAX, reverse=reverse, lens=ln, x=x, vI=None, iW=iW, sW=sW, sW2=sW2, b=b,
                  h=h, zr=zr, h22=h22, zr22=zr22, cap=R.CAP)


@functools.lru_cache(maxsize=None)
def stack_case(n, nlayer, T, lens_on):
    layers = [tile_weights(n, n, k + 1) for k in range(nlayer)]
    x = np.ascontiguousarray(tile_input(n)[:T])
    ln = np.asarray(ragged(T), np.int32) if lens_on else None
    return R.Case(I=n, n=n, regime="moderate", T=T, B=BMAX, reverse=None, lens=ln, x=x, vI=None, layers=layers,
                  h=R.gru_stack(x, layers, ln), zr=None, h22=R.gru_stack(x, layers, ln, R.F32, 22), zr22=None, cap=R.CAP * nlayer)


def same_bits(a, b, what):
    same = a.view(np.uint32) == b.view(np.uint32)
    assert same.all(), "%s differs at %s: %s against %s" % (what, np.argwhere(~same)[:4].tolist(), a[~same][:4], b[~same][:4])


def launch(L, plan, xd, wd, T, B, I, n, reverse, ld, save):
    import torch
    from tests.gpu_util import stream
    y = torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda")
    zr = torch.full((T, B, 2 * n), FILL, dtype=torch.float32, device="cuda") if save else None
    iW, sW, sW2, b = wd
    rc = L.slk_gru_bar16_f32(xd.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.data_ptr(), n, T, B, I, n,
                             int(reverse) | plan, 1, 2, None if ld is None else ld.data_ptr(), None if zr is None else zr.data_ptr(), stream())
    assert rc == 0, rc
    return y.cpu().numpy(), None if zr is None else zr.cpu().numpy()


def geometries():
    for T in TS:
        for B in BS:
            for reverse in (False, True):
                for lens_on in (False, True):
                    yield T, B, reverse, lens_on


@pytest.mark.parametrize("I,n", SHAPES)
def test_every_projection_tile_of_a_layer_launch(I, n):
    from tests.gpu_util import dev, need_gpu
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    wd = tuple(dev(a) for a in tile_weights(I, n))
    for T, B, reverse, lens_on in geometries():
        case = layer_case(I, n, T, reverse, lens_on).take(B)
        xd = dev(case["x"])
        ld = None if case["lens"] is None else dev(case["lens"])
        what = "%d->%d T=%d B=%d reverse=%d ragged=%d" % (I, n, T, B, reverse, lens_on)
        h4, _ = launch(L, PLAN_FOUR, xd, wd, T, B, I, n, reverse, ld, False)
        h4s, zr4 = launch(L, PLAN_FOUR, xd, wd, T, B, I, n, reverse, ld, True)
        h8, zr8 = launch(L, PLAN_EIGHT, xd, wd, T, B, I, n, reverse, ld, True)
        R.check(h4, None, case, what + " plain")
        R.check(h4s, zr4, case, what + " saved gates")
        same_bits(h4, h8, what + ": h, four chunks against eight")
        same_bits(h4s, h8, what + ": h with saved gates, four chunks against eight")
        same_bits(zr4, zr8, what + ": z | r, four chunks against eight")


def run_stack(L, packs, xd, T, B, n, ld):
    """One stack launch of len(packs) layers, reversed first; -> the layers' outputs in order."""
    import torch
    from sloika_amd import _lib
    from tests.gpu_util import stream
    outs = [torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda") for _ in packs]
    descs = (_lib.GruStackLayer * len(packs))()
    cur = xd
    for k, pk in enumerate(packs):
        descs[k] = _lib.GruStackLayer(cur.data_ptr(), n, outs[k].data_ptr(), n, pk.data_ptr(),
                                      ((k + 1) & 1) | (_lib.SLK_GRU_STACK_NO_LENS if ld is None else 0), 0)
        cur = outs[k]
    rc = L.slk_gru_bar16_stack_f32(len(packs), descs, n, n, T, B, None if ld is None else ld.data_ptr(), stream())
    assert rc == 0, rc
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("nlayer", [1, 3])
def test_every_projection_tile_of_packed_and_stacked_layers(nlayer):
    """nlayer = 1: the packed layer.  nlayer = 3: layers 2 and 3 take their images behind a layer boundary, from another pack."""
    from tests.gpu_util import dev, need_gpu, stream
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    n = 96
    ws, packs = [], []
    for k in range(nlayer):
        wd = tuple(dev(a) for a in tile_weights(n, n, k + 1))
        pk = torch.empty(L.slk_gru_bar16_pack_bytes(n, n), dtype=torch.uint8, device="cuda")
        assert pk.numel() > 0
        assert L.slk_gru_bar16_pack_f32(wd[0].data_ptr(), wd[3].data_ptr(), wd[1].data_ptr(), wd[2].data_ptr(), n, n, pk.data_ptr(), stream()) == 0
        ws.append(wd)
        packs.append(pk)
    for T in TS:
        for B in BS:
            for lens_on in (False, True):
                case = stack_case(n, nlayer, T, lens_on).take(B)
                xd = dev(case["x"])
                ld = None if case["lens"] is None else dev(case["lens"])
                what = "%d layers T=%d B=%d ragged=%d" % (nlayer, T, B, lens_on)
                outs = run_stack(L, packs, xd, T, B, n, ld)
                R.check(outs[-1], None, case, what)
                cur = xd
                for k in range(nlayer):                               # the same layers, one eight-chunk launch each
                    want, _ = launch(L, PLAN_EIGHT, cur, ws[k], T, B, n, n, (k + 1) & 1, ld, False)
                    same_bits(outs[k], want, what + ": layer %d, stack against eight-chunk launches" % (k + 1))
                    cur = dev(want)


def test_projection_tiles_repeat_with_every_cu_busy():
    """Fifty groups, a workgroup on every CU, five launches per direction: the same bits each time, and the eight-chunk plan's."""
    from tests.gpu_util import dev, need_gpu
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    I = n = 96
    T, B = 200, 1024
    wd = tuple(dev(a) for a in tile_weights(I, n))
    x = (np.random.RandomState(9).randint(-32768, 32768, size=(T, B, I)) / 16384.0).astype(np.float32)
    xd = dev(x)
    for reverse in (False, True):
        want, _ = launch(L, PLAN_EIGHT, xd, wd, T, B, I, n, reverse, None, False)
        for rep in range(5):
            got, _ = launch(L, PLAN_FOUR, xd, wd, T, B, I, n, reverse, None, False)
            same_bits(got, want, "reverse=%d launch %d" % (reverse, rep))
