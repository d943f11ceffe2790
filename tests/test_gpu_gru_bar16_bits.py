"""csrc/gru_bar16.hip (the four-chunk plan of slk_gru_bar16_f32, forced with bits 8-9 of `reverse`) against its own recorded results,
bit for bit (tests/golden/gru_bar16_bits.npz, written by tools/gru_bits_record.py from the kernel as it stood before the recurrent
MFMAs took the state as their A operand: design/gru_transposed.md).

A change of which lane holds which (neuron, chunk) pair, of the order in which a wave issues the MFMAs of different accumulators, or
of how a gate's pre-activation is gathered from an accumulator must not move a bit: every accumulator sees the same products in the
same order and the hi + lo sum adds the same two values.  tests/test_gpu_gru_bar16.py compares with the oracle at 2e-5 and with the
eight-chunk plan bit for bit (gru_bar16d.hip: another kernel that could be changed in the same way at the same time); this file
pins the four-chunk kernel to itself.

Cases: the seven (I, N) instantiations x T in {1, 3, 4, 5, 9} (one step, a projection group of four not full, full, full + 1, two
groups + 1) x B in {1, 3, 4, 5} (a lone chunk, a partly dead workgroup, a full one, a second workgroup with one live chunk) x
{forward, reversed} x {full, ragged lengths} x {without, with the saved gates: the SAVE instantiation}.  Per case: CRC32 of h_out
and of zr_out (rows the kernel leaves untouched keep the fill value and are part of the sum), and -- from the run without saved
gates -- the first and the last row of h_out as floats, so that a failure shows numbers and not only two checksums.

Inputs are numpy integers scaled by powers of two (no libm call), so that they are the same bits on every host and the results
depend on this kernel alone."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_bar16_bits.npz")
SHAPES = [(96, 96), (64, 64), (32, 96), (128, 96), (64, 96), (48, 32), (16, 64)]
TS = (1, 3, 4, 5, 9)
BS = (1, 3, 4, 5)
FILL = -5.0                           # what h_out / zr_out hold where the kernel stores nothing (rows past a chunk's length)
PLAN_FOUR = 1 << 8                    # include/sloika_amd.h: bits 8-9 of `reverse` = 1 -> four chunks per workgroup


def cases():
    """(T, B, reverse, ragged, save) in the order the golden file stores them."""
    return [(T, B, rev, ragged, save) for T in TS for B in BS for rev in (0, 1) for ragged in (False, True) for save in (False, True)]


def shape_inputs(I, n):
    """Weights of a layer and x for the largest case (the others take its leading steps and chunks): integers / powers of two.
    |x| < 2, |iW| < 1/8, |sW|, |sW2| < 1/4, |b| < 1: pre-activations of order one, gates neither saturated nor flat."""
    rs = np.random.RandomState(7000 + 131 * I + n)
    iW = (rs.randint(-4096, 4096, size=(3 * n, I)) / 32768.0).astype(np.float32)
    sW = (rs.randint(-4096, 4096, size=(2 * n, n)) / 16384.0).astype(np.float32)
    sW2 = (rs.randint(-4096, 4096, size=(n, n)) / 16384.0).astype(np.float32)
    b = (rs.randint(-4096, 4096, size=3 * n) / 4096.0).astype(np.float32)
    x = (rs.randint(-32768, 32768, size=(max(TS), max(BS), I)) / 16384.0).astype(np.float32)
    return iW, sW, sW2, b, x


def case_lens(I, n, T, B):
    return np.random.RandomState(100000 * I + 1000 * n + 10 * T + B).randint(1, T + 1, size=B).astype(np.int32)


def run_shape(I, n):
    """Every case of one instantiation: (crc of h_out, crc of zr_out or 0, first row, last row) per case, as numpy arrays."""
    import torch
    from sloika_amd import _lib
    from tests.gpu_util import dev, stream
    L = _lib.lib()
    iW, sW, sW2, b, xall = shape_inputs(I, n)
    iWd, sWd, sW2d, bd = dev(iW), dev(sW), dev(sW2), dev(b)
    out = []
    for (T, B, rev, ragged, save) in cases():
        xd = dev(xall[:T, :B])
        ld = dev(case_lens(I, n, T, B)) if ragged else None
        y = torch.full((T, B, n), FILL, dtype=torch.float32, device="cuda")
        zr = torch.full((T, B, 2 * n), FILL, dtype=torch.float32, device="cuda") if save else None
        rc = L.slk_gru_bar16_f32(xd.data_ptr(), I, iWd.data_ptr(), sWd.data_ptr(), sW2d.data_ptr(), bd.data_ptr(), y.data_ptr(), n, T, B,
                                 I, n, rev | PLAN_FOUR, 1, 2, None if ld is None else ld.data_ptr(), None if zr is None else zr.data_ptr(),
                                 stream())
        assert rc == 0, (I, n, T, B, rev, ragged, save, rc)
        h = y.cpu().numpy()
        hcrc = zlib.crc32(np.ascontiguousarray(h).tobytes()) & 0xFFFFFFFF
        zcrc = (zlib.crc32(np.ascontiguousarray(zr.cpu().numpy()).tobytes()) & 0xFFFFFFFF) if save else 0
        out.append((hcrc, zcrc, h[0, 0].copy(), h[T - 1, B - 1].copy()))
    return out


def record(I, n):
    """What the golden file holds for one instantiation (rows only from the cases without saved gates, in the order of cases())."""
    res = run_shape(I, n)
    rows = [(f, l) for (f, l), c in zip(((r[2], r[3]) for r in res), cases()) if not c[4]]
    tag = "%d_%d" % (I, n)
    return {"hcrc_" + tag: np.array([r[0] for r in res], dtype=np.uint32), "zcrc_" + tag: np.array([r[1] for r in res], dtype=np.uint32),
            "first_" + tag: np.stack([f for f, _ in rows]).astype(np.float32), "last_" + tag: np.stack([l for _, l in rows]).astype(np.float32)}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_FILE))


@pytest.mark.parametrize("I,n", SHAPES)
def test_four_chunk_gru_keeps_its_recorded_bits(golden, I, n):
    from tests.gpu_util import need_gpu
    need_gpu()
    tag = "%d_%d" % (I, n)
    hcrc, zcrc, first, last = (golden[k + tag] for k in ("hcrc_", "zcrc_", "first_", "last_"))
    res = run_shape(I, n)
    assert len(res) == len(cases()) == hcrc.size == zcrc.size and first.shape == last.shape == (len(res) // 2, n)
    ri = 0
    for ci, ((T, B, rev, ragged, save), (hc, zc, f, l)) in enumerate(zip(cases(), res)):
        what = "%d->%d T=%d B=%d reverse=%d ragged=%s saved gates=%s" % (I, n, T, B, rev, ragged, save)
        if not save:
            # the rows first (as bits): a failure prints the floats that moved
            assert np.array_equal(f.view(np.uint32), first[ri].view(np.uint32)), "%s: first row\n%s\nrecorded\n%s" % (what, f, first[ri])
            assert np.array_equal(l.view(np.uint32), last[ri].view(np.uint32)), "%s: last row\n%s\nrecorded\n%s" % (what, l, last[ri])
            ri += 1
        assert hc == int(hcrc[ci]), "%s: h_out" % what
        assert zc == int(zcrc[ci]), "%s: zr_out" % what
    assert ri == first.shape[0]
