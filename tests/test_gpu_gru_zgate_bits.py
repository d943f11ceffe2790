"""The four-chunk Gru kernel (csrc/gru_bar16_body.h: per layer unpacked, per layer from a pack, five layers in one launch, and the
SAVE instantiation that also writes the gates) against its own recorded results, bit for bit: tests/golden/gru_zgate_bits.npz,
written by tools/gru_zgate_record.py from the library as it stood BEFORE the update gate's products were moved inside the step
(design/gru_zgate.md).  Where in a step a wave issues the z MFMAs, and which wave forms sigmoid(z), must not move a bit: every z
accumulator sees the same products in the same order, the pick adds the same two registers, fmaf and sigmoid keep their operands.

Cases: (I, N) in 96->96, 64->64, 128->96, 16->64 x T' in {1, 2, 3, 4, 5, 8, 9, 17} (inside the four-step group, the group, the two
groups of the prologue, a group plus one, four groups plus one) x B in {1, 4, 5} (a workgroup with dead slots, a full one, a second
workgroup with one live chunk) x {forward, reversed} x {full, ragged lengths with one chunk of length 1}
  * plain:  slk_gru_bar16_f32, four-chunk plan (PACKED = false), every shape;
  * packed: slk_gru_bar16_stack_f32 with one layer (PACKED = true), the two packed shapes;
  * save:   slk_gru_bar16_f32 with zr_out (SAVE), 96->96;
  * stack:  five layers of alternating direction in one launch at T' = 9, the two packed shapes x B x {full, ragged}.
Per case the file holds the CRC32 of ALL of h_out (and zr_out, and the stack's two intermediate buffers) -- rows the kernel leaves
untouched keep the fill value and are part of the sum -- and, as float32 bit patterns, the first row of the first chunk and the last
row of the last chunk, so that a failure shows numbers.  (Every output in full would be 6 MB: six times what a committed file may be.)

Inputs are numpy integers scaled by powers of two (no libm call): the same bits on every host."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_zgate_bits.npz")
SHAPES = [(96, 96), (64, 64), (128, 96), (16, 64)]
PACKED_SHAPES = [(96, 96), (64, 64)]
SAVE_SHAPES = [(96, 96)]
TS = (1, 2, 3, 4, 5, 8, 9, 17)
BS = (1, 4, 5)
STACK_T, STACK_LAYERS = 9, 5
FILL = -5.0                           # what the outputs hold where the kernel stores nothing (rows past a chunk's length)
PLAN_FOUR = 1 << 8                    # include/sloika_amd.h: bits 8-9 of `reverse` = 1 -> four chunks per workgroup
RUNS = [("plain", I, n) for I, n in SHAPES] + [("packed", I, n) for I, n in PACKED_SHAPES] + [("save", I, n) for I, n in SAVE_SHAPES] + \
       [("stack", I, n) for I, n in PACKED_SHAPES]


def cases(mode):
    """(T, B, reverse, ragged) in the order the golden file stores them (stack: reverse = direction of the FIRST layer)."""
    ts = (STACK_T,) if mode == "stack" else TS
    return [(T, B, rev, ragged) for T in ts for B in BS for rev in (0, 1) for ragged in (False, True)]


def layer_weights(I, n, k=0):
    """Layer k: |iW| < 1/8, |sW|, |sW2| < 1/4, |b| < 1: pre-activations of order one, gates neither saturated nor flat."""
    rs = np.random.RandomState(5000 + 131 * I + n + 17 * k)
    iW = (rs.randint(-4096, 4096, size=(3 * n, I)) / 32768.0).astype(np.float32)
    sW = (rs.randint(-4096, 4096, size=(2 * n, n)) / 16384.0).astype(np.float32)
    sW2 = (rs.randint(-4096, 4096, size=(n, n)) / 16384.0).astype(np.float32)
    b = (rs.randint(-4096, 4096, size=3 * n) / 4096.0).astype(np.float32)
    return iW, sW, sW2, b


def shape_input(I, n):
    """x of the largest case; the others take its leading steps and chunks."""
    return (np.random.RandomState(300 + 7 * I + n).randint(-32768, 32768, size=(max(TS), max(BS), I)) / 16384.0).astype(np.float32)


def case_lens(I, n, T, B):
    lens = np.random.RandomState(100000 * I + 1000 * n + 10 * T + B).randint(1, T + 1, size=B).astype(np.int32)
    lens[B // 2] = 1                                                  # a chunk of length 1
    return lens


def crc(t):
    return zlib.crc32(np.ascontiguousarray(t.cpu().numpy()).tobytes()) & 0xFFFFFFFF


def run_mode(mode, I, n):
    """Every case of one run: per case (crcs: h_out, then zr_out or the stack's two buffers or 0, 0; rows: first of h_out, last of
    h_out, and with saved gates first and last of zr_out), as numpy arrays."""
    import torch
    from sloika_amd import _lib
    from tests.gpu_util import dev, stream
    L = _lib.lib()
    nl = STACK_LAYERS if mode == "stack" else 1
    ws = [tuple(dev(a) for a in layer_weights(I, n, k)) for k in range(nl)]
    packs = []
    if mode in ("packed", "stack"):
        for iW, sW, sW2, b in ws:
            pk = torch.empty(L.slk_gru_bar16_pack_bytes(I, n), dtype=torch.uint8, device="cuda")
            assert pk.numel() > 0
            assert L.slk_gru_bar16_pack_f32(iW.data_ptr(), b.data_ptr(), sW.data_ptr(), sW2.data_ptr(), I, n, pk.data_ptr(), stream()) == 0
            packs.append(pk)
    xall = shape_input(I, n)
    out = []
    for (T, B, rev, ragged) in cases(mode):
        xd = dev(xall[:T, :B])
        ld = dev(case_lens(I, n, T, B)) if ragged else None
        y = torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda")
        extra = []
        if mode in ("plain", "save"):
            iW, sW, sW2, b = ws[0]
            zr = torch.full((T, B, 2 * n), FILL, dtype=torch.float32, device="cuda") if mode == "save" else None
            rc = L.slk_gru_bar16_f32(xd.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.data_ptr(), n, T, B,
                                     I, n, rev | PLAN_FOUR, 1, 2, None if ld is None else ld.data_ptr(), None if zr is None else zr.data_ptr(),
                                     stream())
            if zr is not None:
                extra = [zr]
        else:
            tmp = [torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda") for _ in range(2)]
            descs = (_lib.GruStackLayer * nl)()
            cur = xd
            for k in range(nl):
                dst = y if k == nl - 1 else tmp[k & 1]
                descs[k] = _lib.GruStackLayer(cur.data_ptr(), I, dst.data_ptr(), n, packs[k].data_ptr(),
                                              ((rev + k) & 1) | (0 if ragged else _lib.SLK_GRU_STACK_NO_LENS), 0)
                cur = dst
            rc = L.slk_gru_bar16_stack_f32(nl, descs, I, n, T, B, None if ld is None else ld.data_ptr(), stream())
            if mode == "stack":
                extra = tmp
        assert rc == 0, (mode, I, n, T, B, rev, ragged, rc)
        h = y.cpu().numpy()
        crcs = [crc(y)] + [crc(t) for t in extra] + [0] * (2 - len(extra))
        rows = [h[0, 0].copy(), h[T - 1, B - 1].copy()]
        if mode == "save":
            z = extra[0].cpu().numpy()
            rows += [z[0, 0].copy(), z[T - 1, B - 1].copy()]
        out.append((crcs, rows))
    return out


def record(mode, I, n):
    """What the golden file holds for one run: crc_<tag> (cases, 3) and row<k>_<tag> (cases, width) as uint32."""
    res = run_mode(mode, I, n)
    tag = "%s_%d_%d" % (mode, I, n)
    data = {"crc_" + tag: np.array([c for c, _ in res], dtype=np.uint32)}
    for k in range(len(res[0][1])):
        data["row%d_%s" % (k, tag)] = np.stack([r[k] for _, r in res]).astype(np.float32).view(np.uint32)
    return data


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_FILE))


@pytest.mark.parametrize("mode,I,n", RUNS)
def test_four_chunk_gru_keeps_the_bits_recorded_before_the_update_gate_moved(golden, mode, I, n):
    from tests.gpu_util import need_gpu
    need_gpu()
    tag = "%s_%d_%d" % (mode, I, n)
    want_crc = golden["crc_" + tag]
    res = run_mode(mode, I, n)
    assert len(res) == len(cases(mode)) == want_crc.shape[0]
    names = ("h_out", "zr_out", "zr_out") if mode == "save" else ("h_out", "first buffer between layers", "second buffer between layers")
    rownames = ("first row of h_out", "last row of h_out", "first row of zr_out", "last row of zr_out")
    for ci, ((T, B, rev, ragged), (crcs, rows)) in enumerate(zip(cases(mode), res)):
        what = "%s %d->%d T'=%d B=%d reverse=%d ragged=%s" % (mode, I, n, T, B, rev, ragged)
        for k, row in enumerate(rows):                  # the rows first (as bits): a failure prints the floats that moved
            want = golden["row%d_%s" % (k, tag)][ci]
            assert np.array_equal(row.view(np.uint32), want), "%s: %s\n%s\nrecorded\n%s" % (what, rownames[k], row, want.view(np.float32))
        for k in range(3):
            assert crcs[k] == int(want_crc[ci, k]), "%s: %s" % (what, names[k])
