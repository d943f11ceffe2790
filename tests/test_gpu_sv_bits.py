"""csrc/softmax_viterbi.hip against its own recorded results, bit for bit (tests/golden/sv_bits.npz, written by
tools/sv_bits_record.py from the kernel as it stood before its production schedule went K-block-major: design/decode_kmajor.md).

A change of the kernel's SCHEDULE -- the order in which a wave requests operands, issues MFMAs of different accumulators, finishes
tiles -- must not move a bit: every accumulator sees the same MFMAs in the same order, the row sums keep ((t0 + t1) + t2) + t3, the
reductions and the dynamic programme keep their arithmetic.  tests/test_gpu_fused_decode.py would let a last-bit change of a
log-posterior through (its tolerance is 2e-5); this file does not.

Cases: insize K of every instantiation (64, 96, 112, 128) x T' in {1, 15, 16, 17, 47} (a single partial block, exactly one block, one
block and a row, three blocks with a ragged end) x batch {1, 3} (an odd batch leaves the second chunk of the last workgroup dead) x
skip penalty {0, 1.5} x {full, ragged lengths}.  Per case: paths, lengths, float32 scores, and a CRC32 of the dumped log-posteriors
(rows of a chunk past its own length are not part of the result and count as zero), from the kernel without the dump and from the
dumping instantiation.

Inputs are made from numpy's uniform generator with float64 products only (no libm call), so that they are the same bits on every
host.  The weights have the standard deviation models.randomise_zero_layers gives a layer (sd = 0.5 truncated normal over
sqrt(fan in + fan out); biases sd 0.5)."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sv_bits.npz")
KS = (64, 96, 112, 128)
TS = (1, 15, 16, 17, 47)
BS = (1, 3)
SKIPS = (0.0, 1.5)
NSTATE = 1025
TRUNC_SD = 0.8796                     # standard deviation of a standard normal truncated to [-2, 2]


def cases(K):
    """(T', B, skip, ragged) of insize K, in the order the golden file stores them."""
    return [(T, B, skip, ragged) for T in TS for B in BS for skip in SKIPS for ragged in (False, True)]


def _uniform_sd1(rs, shape):
    return (rs.random_sample(size=shape) * 2.0 - 1.0) * np.sqrt(3.0)


def softmax_weights(K, sd=0.5):
    rs = np.random.RandomState(9100 + K)
    W = (sd * TRUNC_SD * _uniform_sd1(rs, (NSTATE, K)) / np.sqrt(float(NSTATE + K))).astype(np.float32)
    b = (sd * TRUNC_SD * _uniform_sd1(rs, NSTATE)).astype(np.float32)
    return W, b


def case_inputs(K, T, B, skip, ragged):
    rs = np.random.RandomState(100000 * K + 1000 * T + 10 * B + int(ragged) + (5 if skip else 0))
    x = (rs.random_sample(size=(T, B, K)) * 2.0 - 1.0).astype(np.float32)
    x[min(3, T - 1)] = 0.0                                               # a row whose logits are just the bias
    lens = rs.randint(1, T + 1, size=B).astype(np.int32) if ragged else None
    return x, lens


def run_case(pack, K, T, B, skip, ragged, dump):
    """(paths, lens, scores, crc32 of the log-posteriors or None) of one case as numpy arrays."""
    import torch
    from sloika_amd import decode
    x, lens = case_inputs(K, T, B, skip, ragged)
    xd = torch.from_numpy(x).cuda()
    ld = torch.from_numpy(lens).cuda() if lens is not None else None
    lp = torch.zeros((T, B, NSTATE), dtype=torch.float32, device="cuda") if dump else None
    sc, pa, le = decode.viterbi_fused_batch(xd, pack, 5, skip_pen=skip, lengths=ld, lp_dump=lp)
    crc = None
    if dump:
        lpn = lp.cpu().numpy()
        if lens is not None:
            for b in range(B):
                lpn[lens[b]:, b] = 0.0
        crc = zlib.crc32(np.ascontiguousarray(lpn).tobytes()) & 0xFFFFFFFF
    return pa.cpu().numpy().copy(), le.cpu().numpy().copy(), sc.cpu().numpy().copy(), crc


def make_pack(K):
    from sloika_amd import layers
    W, b = softmax_weights(K)
    sm = layers.Softmax(K, NSTATE, has_bias=True)
    sm.W.set_value(W)
    sm.b.set_value(b)
    pack = sm.viterbi_pack(4, 5)
    assert pack is not None
    return pack


def record(K):
    """What the golden file holds for insize K: the cases' results concatenated in the order of cases(K)."""
    pack = make_pack(K)
    paths, lens, scores, crcs = [], [], [], []
    for (T, B, skip, ragged) in cases(K):
        pa, le, sc, crc = run_case(pack, K, T, B, skip, ragged, dump=True)
        paths.append(pa.ravel())
        lens.append(le)
        scores.append(sc)
        crcs.append(crc)
    return {"paths_%d" % K: np.concatenate(paths).astype(np.int32), "lens_%d" % K: np.concatenate(lens).astype(np.int32),
            "scores_%d" % K: np.concatenate(scores).astype(np.float32), "lpcrc_%d" % K: np.array(crcs, dtype=np.uint32)}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_FILE))


@pytest.mark.parametrize("K", KS)
def test_fused_decoder_keeps_its_recorded_bits(golden, K):
    from tests.gpu_util import need_gpu
    need_gpu()
    pack = make_pack(K)
    gp, gl, gs, gc = (golden["%s_%d" % (n, K)] for n in ("paths", "lens", "scores", "lpcrc"))
    po = bo = 0
    for ci, (T, B, skip, ragged) in enumerate(cases(K)):
        want_p, want_l, want_s = gp[po:po + B * T].reshape(B, T), gl[bo:bo + B], gs[bo:bo + B]
        po, bo = po + B * T, bo + B
        for dump in (False, True):                                       # softmax_viterbi_kernel<KS, false> and <KS, true>
            pa, le, sc, crc = run_case(pack, K, T, B, skip, ragged, dump)
            what = "K=%d T'=%d B=%d skip=%g ragged=%s dump=%s" % (K, T, B, skip, ragged, dump)
            assert np.array_equal(le, want_l), what
            assert np.array_equal(pa, want_p), what
            assert np.array_equal(sc.view(np.uint32), want_s.view(np.uint32)), what    # float32 scores as bits
            if dump:
                assert crc == int(gc[ci]), what
    assert po == gp.size and bo == gl.size
