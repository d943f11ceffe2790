"""The full-batch instantiation of the four-chunk stack kernel (csrc/gru_bar16_body.h: FULL; design/gru_store.md): a launch of
slk_gru_bar16_stack_f32 in which no layer looks at lens, with B % 4 == 0, stores h without a predicate.  Every other launch takes the
general kernel.  Nothing about the values may differ: the same bits at the same addresses, and nothing written anywhere else.

How the two are told apart from outside: the same batch with a `lens` array that holds T' everywhere (and layers that look at it)
is ragged as far as the launcher can know, and takes the general kernel; slk_gru_bar16_stack_path names the choice.  The yardstick
of both is the eight-chunk plan of slk_gru_bar16_f32 (plan bits 2: another kernel file, documented as bit-identical), layer by layer
on the same operands, and for the batches that never take FULL also the float64 recursion of tests/ref_gru_forward.py under its
bound.  Outputs are the NaN-canaried buffers of tests/gpu_util.py: guards, padding columns and rows >= T' must keep their pattern.

T' in {1, 2, 3, 4, 5, 8, 9}: every phase of the group loop as the last step (T' = 1, 2, 3, 4 -> phases 0 to 3; 5 and 9 -> phase 0
behind a full group, where the store of h(s-1) in phase 0 is the uniform test of the group counter), and the ring turnover 8 | 9."""
import functools

import numpy as np
import pytest

from tests import ref_gru_forward as rg
from tests.gpu_util import Out, dev, need_gpu, stream

pytestmark = pytest.mark.gpu

TS = (1, 2, 3, 4, 5, 8, 9)
FULL_B = (4, 8, 12)
OTHER_B = (1, 5, 9)
SIZES = (96, 64)
MAXL = 3


def _L():
    need_gpu()
    from sloika_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _layers(n):
    """Host weights, device weights and packs of the MAXL layers of an n -> n stack."""
    import torch
    L = _L()
    host = rg.stack_weights(n, MAXL)
    devw, packs = [], []
    for iW, sW, sW2, b in host:
        d = [dev(a) for a in (iW, sW, sW2, b)]
        pk = torch.empty(L.slk_gru_bar16_pack_bytes(n, n), dtype=torch.uint8, device="cuda")
        assert pk.numel() > 0
        assert L.slk_gru_bar16_pack_f32(d[0].data_ptr(), d[3].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, n, pk.data_ptr(), stream()) == 0
        devw.append(d)
        packs.append(pk)
    torch.cuda.synchronize()
    return host, devw, packs


@functools.lru_cache(maxsize=None)
def _x(n, T):
    return rg.inputs(n, T, max(FULL_B), 17 * n + T)


def _outs(nlayer, T, B, n, ldh, lead, rows):
    return [Out(rows or T, B, n, ldh, lead) for _ in range(nlayer)]


def run_stack(n, nlayer, start_rev, xd, T, B, lens=None, tell="all", ldh=None, lead=0, rows=None):
    """One slk_gru_bar16_stack_f32 launch, every layer into a canaried buffer of its own -> the fetched buffers.  lens: told to every
    layer (tell = "all") or to the reversed ones only ("reversed", what sloika_amd.layers does)."""
    import torch
    from sloika_amd import _lib
    L = _L()
    _, _, packs = _layers(n)
    outs = _outs(nlayer, T, B, n, ldh, lead, rows)
    descs = (_lib.GruStackLayer * nlayer)()
    cur, ldcur = xd.data_ptr(), n
    for k in range(nlayer):
        rev = int(start_rev) ^ (k & 1)
        nolens = lens is None or (tell == "reversed" and not rev)
        descs[k] = _lib.GruStackLayer(cur, ldcur, outs[k].ptr(), outs[k].ld, packs[k].data_ptr(),
                                      rev | (_lib.SLK_GRU_STACK_NO_LENS if nolens else 0), 0)
        cur, ldcur = outs[k].ptr(), outs[k].ld
    rc = L.slk_gru_bar16_stack_f32(nlayer, descs, n, n, T, B, None if lens is None else lens.data_ptr(), stream())
    assert rc == 0, (n, nlayer, T, B, rc)
    torch.cuda.synchronize()
    return [o.fetch() for o in outs]


def run_chain(n, nlayer, start_rev, xd, T, B, plan, lens=None, tell="all", ldh=None, lead=0, rows=None):
    """The same layers as slk_gru_bar16_f32 launches of the given plan, one per layer."""
    import torch
    L = _L()
    _, devw, _ = _layers(n)
    outs = _outs(nlayer, T, B, n, ldh, lead, rows)
    cur, ldcur = xd.data_ptr(), n
    for k in range(nlayer):
        rev = int(start_rev) ^ (k & 1)
        nolens = lens is None or (tell == "reversed" and not rev)
        iW, sW, sW2, b = devw[k]
        rc = L.slk_gru_bar16_f32(cur, ldcur, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), outs[k].ptr(), outs[k].ld, T, B,
                                 n, n, rev | (plan << 8), 1, 2, None if nolens else lens.data_ptr(), None, stream())
        assert rc == 0, (n, k, T, B, plan, rc)
        cur, ldcur = outs[k].ptr(), outs[k].ld
    torch.cuda.synchronize()
    return [o.fetch() for o in outs]


def _same_bytes(a, b, what):
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p.host, q.host), "%s: layer %d differs" % (what, k)


# ------------------------------------------------------------------------------------- FULL against today's path, bit for bit
@pytest.mark.parametrize("start_rev", [False, True])
@pytest.mark.parametrize("nlayer", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_full_batch_gives_the_bytes_of_the_general_kernel(n, nlayer, start_rev):
    L = _L()
    for T in TS:
        for B in FULL_B:
            what = "n=%d layers=%d start_rev=%d T=%d B=%d" % (n, nlayer, start_rev, T, B)
            assert L.slk_gru_bar16_stack_path(B, 0) == 1 and L.slk_gru_bar16_stack_path(B, 1) == 0, what
            xd = dev(_x(n, T)[:, :B])
            full = run_stack(n, nlayer, start_rev, xd, T, B)
            told = run_stack(n, nlayer, start_rev, xd, T, B, lens=dev(np.full(B, T, np.int32)))
            eight = run_chain(n, nlayer, start_rev, xd, T, B, 2)
            for o in full + told + eight:
                o.assert_untouched_outside(None, what)
            _same_bytes(full, told, what + " FULL | lens = T' everywhere")
            _same_bytes(full, eight, what + " FULL | eight-chunk plan")
            for k in range(nlayer):                                   # the first and the last row of either direction, by name
                for row in (0, T - 1):
                    assert np.array_equal(full[k].body()[row], eight[k].body()[row]), (what, k, row)
            if nlayer == 1:
                _same_bytes(full, run_chain(n, 1, start_rev, xd, T, B, 1), what + " FULL | four-chunk layer kernel")


# --------------------------------------------------------------------------------------------- batches that must not take FULL
@functools.lru_cache(maxsize=None)
def _case(n, nlayer, T, B, lens):
    """float64 and y22 of a stack of rg.stack_weights, directions alternating and starting reversed (rg.gru_stack)."""
    layers = rg.stack_weights(n, MAXL)[:nlayer]
    x = np.ascontiguousarray(_x(n, T)[:, :B])
    ln = None if lens is None else np.asarray(lens, np.int32)
    return rg.Case(I=n, n=n, regime="moderate", T=T, B=B, reverse=None, lens=ln, x=x, vI=None, layers=layers,
                   h=rg.gru_stack(x, layers, ln), zr=None, h22=rg.gru_stack(x, layers, ln, rg.F32, 22), zr22=None, cap=rg.CAP * nlayer)


def _own_rows(o, lens, T):
    """The rows of each chunk's own steps (the others are canaries, or NaN a forward layer made of canaries)."""
    v = o.values()
    keep = np.arange(T)[:, None] < (np.full(v.shape[1], T) if lens is None else np.asarray(lens))[None, :]
    return v[keep].view(np.uint32)


@pytest.mark.parametrize("nlayer", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_partial_and_ragged_batches_keep_the_general_kernel(n, nlayer):
    L = _L()
    for T in TS:
        ragged = (T, max(T - 1, 1), max(T - 2, 1), max(T - 3, 1), 1)     # workgroup 0: T', T'-1, T'-2, T'-3; workgroup 1: length 1
        for B, lens in [(B, None) for B in OTHER_B] + [(5, ragged)]:
            what = "n=%d layers=%d T=%d B=%d ragged=%d" % (n, nlayer, T, B, lens is not None)
            assert L.slk_gru_bar16_stack_path(B, int(lens is not None)) == 0, what
            c = _case(n, nlayer, T, B, lens)
            xd = dev(c["x"])
            ld = None if lens is None else dev(np.asarray(lens, np.int32))
            got = run_stack(n, nlayer, True, xd, T, B, lens=ld, tell="reversed")
            eight = run_chain(n, nlayer, True, xd, T, B, 2, lens=ld, tell="reversed")
            for k in range(nlayer):
                lk = lens if (k & 1) == 0 else None                      # layer k is reversed for even k: only those leave rows alone
                got[k].assert_untouched_outside(lk, what)
                assert np.array_equal(_own_rows(got[k], lens, T), _own_rows(eight[k], lens, T)), (what, k)
            rg.check(got[-1].values(), None, c, "stack " + what, "stack")


# --------------------------------------------------------------------------------------------- what the new stores may touch
@pytest.mark.parametrize("n", SIZES)
def test_padded_rows_and_a_base_that_is_not_line_aligned(n):
    """ldh in {n, n + 4, n + 8}, the outputs 16 bytes past a 128-byte boundary, two rows more than T' in every buffer: the stores
    write columns 0 .. n-1 of rows 0 .. T'-1 and nothing else."""
    L = _L()
    T, B = 5, 8
    xd = dev(_x(n, T)[:, :B])
    lens = [T] * B
    for ldh in (n, n + 4, n + 8):
        for start_rev in (False, True):
            what = "n=%d ldh=%d start_rev=%d" % (n, ldh, start_rev)
            assert L.slk_gru_bar16_stack_path(B, 0) == 1
            full = run_stack(n, MAXL, start_rev, xd, T, B, ldh=ldh, lead=4, rows=T + 2)
            told = run_stack(n, MAXL, start_rev, xd, T, B, lens=dev(np.asarray(lens, np.int32)), ldh=ldh, lead=4, rows=T + 2)
            eight = run_chain(n, MAXL, start_rev, xd, T, B, 2, ldh=ldh, lead=4, rows=T + 2)
            for o in full + told + eight:
                assert o.ptr() % 128 == 16
                o.assert_untouched_outside(lens, what)
                assert not (o.body()[:T, :, :n] == 0x7FC0BEEF).any(), what
            _same_bytes(full, told, what)
            _same_bytes(full, eight, what)


def test_the_launcher_names_its_path():
    """slk_gru_bar16_stack_path with made-up sizes (host only): FULL needs a launch in which no layer looks at lens, and B % 4 == 0.
    (The variant whose stores address a row through a 32-bit lane offset, and with it the refusal of launches whose B * ldh * 4 does
    not fit 31 bits, was measured and not kept: design/gru_store.md, tools/experiments/gru_store_variants.patch.txt.)"""
    L = _L()
    path = L.slk_gru_bar16_stack_path
    assert path(1024, 0) == 1 and path(1024, 1) == 0
    assert [path(B, 0) for B in (1, 2, 3, 4, 5, 1023, 1025, 1028, 1 << 30)] == [0, 0, 0, 1, 0, 0, 0, 1, 1]
    assert [path(B, 1) for B in (4, 8, 1028)] == [0, 0, 0]
    assert path(0, 0) == 0 and path(-4, 0) == 0
