"""slk_gru_bar16_stack_f32 (csrc/gru_bar16.hip: weight images from a pack made once, several layers in one launch) against the kernel
it is made of, bit for bit.

  * one layer from its pack == slk_gru_bar16_f32 (four-chunk plan) on the same operands: the pack kernel makes the images with the
    functions the layer kernel's prologue calls, so the images, and with them every product, are the same bits;
  * nlayer layers in one launch == a chain of nlayer slk_gru_bar16_f32 launches through the same buffers: a workgroup reads and writes
    the rows of its own four chunks only, the launch boundary between two layers carries nothing the data needs.

Cases: (96,96) and (64,64) x nlayer in {1, 2, 5}, directions alternating and starting reversed x T in {1, 3, 4, 5, 9} (one step, a
projection group of four not full, full, full + 1, two groups + 1: the waves of a workgroup must meet at the layer boundary whatever T
is) x B in {1, 4, 5, 9} (a lone chunk with three dead slots, a full workgroup, a second / third workgroup with one live chunk) x
{no lengths, ragged lengths told to every layer, ragged lengths told to the reversed layers only (what sloika_amd.layers does)}.
Ragged lengths always hold a chunk of length 1.  Compared: the last layer's output and the two buffers the layers in between write
in turn, every byte (rows no layer stores keep the fill value).

The last test goes through sloika_amd.layers: a Serial of Gru layers takes the stack entry, and after set_params on one of them the
next run gives the new weights' result -- the pack is keyed on the weights' versions.

Inputs are numpy integers scaled by powers of two (no libm call): the same bits on every host."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = (1, 3, 4, 5, 9)
BS = (1, 4, 5, 9)
FILL = -5.0
PLAN_FOUR = 1 << 8                    # include/sloika_amd.h: bits 8-9 of `reverse` = 1 -> four chunks per workgroup
MAXL = 5


def layer_weights(n, k, salt=0):
    """Layer k of an n -> n stack: |iW| < 1/8, |sW|, |sW2| < 1/4, |b| < 1 (pre-activations of order one)."""
    rs = np.random.RandomState(9000 + 131 * n + 17 * k + salt)
    iW = (rs.randint(-4096, 4096, size=(3 * n, n)) / 32768.0).astype(np.float32)
    sW = (rs.randint(-4096, 4096, size=(2 * n, n)) / 16384.0).astype(np.float32)
    sW2 = (rs.randint(-4096, 4096, size=(n, n)) / 16384.0).astype(np.float32)
    b = (rs.randint(-4096, 4096, size=3 * n) / 4096.0).astype(np.float32)
    return iW, sW, sW2, b


def stack_input(n):
    return (np.random.RandomState(77 + n).randint(-32768, 32768, size=(max(TS), max(BS), n)) / 16384.0).astype(np.float32)


def case_lens(n, T, B):
    lens = np.random.RandomState(1000 * n + 10 * T + B).randint(1, T + 1, size=B).astype(np.int32)
    lens[B // 2] = 1                                                  # a chunk of length 1
    return lens


@pytest.fixture(scope="module")
def operands():
    """Per width: the device weights and packs of MAXL layers and the input of the largest case, made once."""
    from tests.gpu_util import dev, need_gpu, stream
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    out = {}
    for n in (96, 64):
        ws, packs = [], []
        for k in range(MAXL):
            iW, sW, sW2, b = (dev(a) for a in layer_weights(n, k))
            pk = torch.empty(L.slk_gru_bar16_pack_bytes(n, n), dtype=torch.uint8, device="cuda")
            assert pk.numel() > 0
            assert L.slk_gru_bar16_pack_f32(iW.data_ptr(), b.data_ptr(), sW.data_ptr(), sW2.data_ptr(), n, n, pk.data_ptr(), stream()) == 0
            ws.append((iW, sW, sW2, b))
            packs.append(pk)
        out[n] = (ws, packs, stack_input(n))
    return out


def run_case(L, n, nlayer, ws, packs, xd, T, B, ld, lens_mode):
    """-> ([final, buffer 0, buffer 1] of the chain of layer launches, the same of the one stack launch), as numpy arrays."""
    import torch
    from sloika_amd import _lib
    from tests.gpu_util import stream
    res = []
    for stacked in (False, True):
        y = torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda")
        tmp = [torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
        descs = (_lib.GruStackLayer * nlayer)()
        cur = xd
        for k in range(nlayer):
            rev = (k + 1) & 1                                         # reversed first, then alternating
            told = ld is not None and (lens_mode == "all" or rev)
            dst = y if k == nlayer - 1 else tmp[k & 1]
            if stacked:
                descs[k] = _lib.GruStackLayer(cur.data_ptr(), n, dst.data_ptr(), n, packs[k].data_ptr(),
                                              rev | (0 if told else _lib.SLK_GRU_STACK_NO_LENS), 0)
            else:
                iW, sW, sW2, b = ws[k]
                rc = L.slk_gru_bar16_f32(cur.data_ptr(), n, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), dst.data_ptr(), n,
                                         T, B, n, n, rev | PLAN_FOUR, 1, 2, ld.data_ptr() if told else None, None, stream())
                assert rc == 0, (n, nlayer, T, B, lens_mode, k, rc)
            cur = dst
        if stacked:
            rc = L.slk_gru_bar16_stack_f32(nlayer, descs, n, n, T, B, None if ld is None else ld.data_ptr(), stream())
            assert rc == 0, (n, nlayer, T, B, lens_mode, rc)
        res.append([t.cpu().numpy() for t in [y] + tmp])
    return res


@pytest.mark.parametrize("nlayer", [1, 2, 5])
@pytest.mark.parametrize("n", [96, 64])
def test_stack_equals_the_chain_of_layer_launches(operands, n, nlayer):
    from sloika_amd import _lib
    from tests.gpu_util import dev
    L = _lib.lib()
    ws, packs, xall = operands[n]
    for T in TS:
        for B in BS:
            xd = dev(xall[:T, :B])
            for lens_mode in (None, "all", "reversed"):
                ld = None if lens_mode is None else dev(case_lens(n, T, B))
                chain, stack = run_case(L, n, nlayer, ws, packs, xd, T, B, ld, lens_mode)
                what = "%d->%d, %d layers, T=%d B=%d lengths: %s" % (n, n, nlayer, T, B, lens_mode)
                assert not np.all(chain[0] == FILL), what              # the reference wrote something
                for name, a, b in zip(("output", "first buffer", "second buffer"), chain, stack):
                    same = a.view(np.uint32) == b.view(np.uint32)
                    assert same.all(), "%s: %s differs at %s\nchain %s\nstack %s" % (what, name, np.argwhere(~same)[:4].tolist(),
                                                                                  a[~same][:4], b[~same][:4])


def test_layers_take_the_stack_and_a_changed_weight_changes_the_result(monkeypatch):
    from tests.gpu_util import dev, need_gpu, stream
    torch = need_gpu()
    from sloika_amd import _lib, layers
    L = _lib.lib()
    n, T, B = 64, 9, 5
    grus = [layers.Gru(n, n, has_bias=True) for _ in range(3)]
    for k, g in enumerate(grus):
        iW, sW, sW2, b = layer_weights(n, k)
        g.set_params({"iW": iW.reshape(3, n, n), "sW": sW.reshape(2, n, n), "sW2": sW2, "b": b.reshape(3, n)})
    net = layers.Serial([layers.Reverse(grus[0]), grus[1], layers.Reverse(grus[2])])
    calls = []
    real = L.slk_gru_bar16_stack_f32
    monkeypatch.setattr(L, "slk_gru_bar16_stack_f32", lambda nl, *a: calls.append(nl) or real(nl, *a))
    xd = dev(stack_input(n)[:T, :B])

    def reference(weights):
        cur = xd
        for k, (iW, sW, sW2, b) in enumerate(weights):
            y = torch.empty((T, B, n), dtype=torch.float32, device="cuda")
            args = [dev(a) for a in (iW, sW, sW2, b)]
            assert L.slk_gru_bar16_f32(cur.data_ptr(), n, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(),
                                       y.data_ptr(), n, T, B, n, n, ((k + 1) & 1) | PLAN_FOUR, 1, 2, None, None, stream()) == 0
            torch.cuda.synchronize()
            cur = y
        return cur.cpu().numpy()

    weights = [layer_weights(n, k) for k in range(3)]
    first = net.run(xd).cpu().numpy()
    assert calls == [3]
    assert np.array_equal(first.view(np.uint32), reference(weights).view(np.uint32))
    again = net.run(xd).cpu().numpy()                                 # the kept packs
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
    weights[1] = layer_weights(n, 1, salt=5)
    iW, sW, sW2, b = weights[1]
    grus[1].set_params({"iW": iW.reshape(3, n, n), "sW": sW.reshape(2, n, n), "sW2": sW2, "b": b.reshape(3, n)})
    second = net.run(xd).cpu().numpy()
    assert calls == [3, 3, 3]
    assert not np.array_equal(second, first)
    assert np.array_equal(second.view(np.uint32), reference(weights).view(np.uint32))
