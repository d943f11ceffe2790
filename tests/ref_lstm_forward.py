"""Plain-numpy restatement of the forward Lstm layer (sloika/layers.py:677-697, zero initial state; Reverse: layers.py:1449-1450),
written from the formulas as a loop of its own, for tests/test_gpu_lstm_forward_edges.py and tests/test_ref_lstm_forward.py.

Three grades of the same recursion, as in tests/ref_gru_forward.py (`BOUND`, `round22`, `sigmoid`, `tanh_one_exp` are those of
tests/ref_reverse_scans.py):
  * float64 (`lstm_forward`): THE reference.  Pinned on the CPU to oracle_np.lstm, the C oracle and the reference's own layer
    outputs under tests/golden/ (tests/test_ref_lstm_forward.py).
  * `y32`: dtype=float32.  The yardstick of slk_lstm_recurrent*_f32 (csrc/lstm_mfma.hip, the portable kernel) and slk_lstm_f32.
  * `y22`: float32 with both operands of x.iW^T and h.sW^T rounded to the 22 significand bits of an fp16 hi + lo pair (a row of x or
    h is one operand vector, a weight row one gate row's weights) -- the precision include/sloika_amd.h promises for
    slk_lstm_fused16_f32, not its code.  For slk_lstm_scan16_f32 the projection vW is handed over and only h.sW^T is rounded.
The float32 grades take tanh as `tanh_one_exp` and the sigmoid in float32: the activation cost csrc/common.h documents.  A
yardstick's distance from float64 is what a kernel of that arithmetic may cost, times `BOUND`.

Ragged batches: with `lens`, chunk b runs over its own lens[b] steps, a reversed scan starts at that chunk's own last step, and
entries at t >= lens[b] come back as MARKER.  Also here: the case generators (fixed seeds), the tables of cases the GPU tests run, and
`check`, the one comparison every GPU test of the forward Lstm goes through."""
import functools
import os
import re

import numpy as np

from tests.ref_gru_forward import chunk_errors, inputs
from tests.ref_reverse_scans import BOUND, round22, sigmoid, tanh_one_exp

F32, F64 = np.float32, np.float64
MARKER = np.nan
#: what the suite already demands of the forward Lstm kernels through their own entries (tests/test_gpu_lstm_fused16.py,
#: tests/test_gpu_lstm_scan16.py, tests/test_gpu_recurrent.py::test_lstm_*: err < 2e-5 against the C oracle)
CAP = 2e-5
#: a case is admitted where its yardstick is at most this: BOUND then sits well inside CAP and the cap never decides
ADMIT = CAP / 8


# ------------------------------------------------------------------------------------------------------- the recursion
def _fair(x):
    return x / (x.dtype.type(1) + np.abs(x) / x.dtype.type(1.3998))           # activation.py:68-69


def _sigmoid_pm(x):
    return np.clip(x.dtype.type(0.5) + x.dtype.type(0.25) * x, x.dtype.type(0), x.dtype.type(1))     # activation.py:88-92


#: name -> (function in float64, function of the float32 grades, id in include/sloika_amd.h).  tanh / sigmoid is what the MFMA and
#: fp16-split kernels take; fair / sigmoid_pm (a division and a clip: nothing a device libm could do differently) is the other pair.
ACTIVATIONS = {"tanh": (np.tanh, tanh_one_exp, 1), "sigmoid": (sigmoid, sigmoid, 2), "fair": (_fair, _fair, 10),
               "sigmoid_pm": (_sigmoid_pm, _sigmoid_pm, 13)}
OTHER_PAIR = ("fair", "sigmoid_pm")


def _product(bits):
    """v[B][K] . W[N][K]^T: as the operands are, or with both at 22 bits."""
    if bits is None:
        return lambda v, W: v @ W.T
    assert bits == 22
    return lambda v, W: round22(v, 1) @ round22(W, 1).T


def lstm_forward(x, iW, sW, b, p, reverse, lens=None, dtype=F64, bits=None, vW=None, act="tanh", gate="sigmoid"):
    """x:[T][B][I] (time order), iW:[4n][I], sW:[4n][n], b:[4n] or None, p:[3][n] or None -> h:[T][B][n].  Gate rows are interleaved,
    row = 4 * unit + gate with gate 0 candidate, 1 input, 2 forget, 3 output.  vW:[T][B][4n], when given, stands for x.iW^T + b (the
    scan entries' input) and x, iW, b are not read.  Per scan step (layers.py:677-691), from c = 0, h = 0:
    a = x iW^T + b + h sW^T;  f = gate(a2 + c p1);  i = gate(a1 + c p0);  c' = c f + act(a0) i;  o = gate(a3 + c' p2);  h' = act(c') o."""
    sW = np.asarray(sW, dtype)
    n = sW.shape[1]
    assert sW.shape == (4 * n, n)
    if vW is None:
        x, iW = np.asarray(x, dtype), np.asarray(iW, dtype)
        bias = np.zeros(4 * n, dtype) if b is None else np.asarray(b, dtype)
        T, B = x.shape[:2]
    else:
        vW = np.asarray(vW, dtype)
        T, B = vW.shape[:2]
    peep = np.zeros((3, n), dtype) if p is None else np.asarray(p, dtype).reshape(3, n)
    grade = 0 if dtype == F64 else 1
    fun, gatefun = ACTIVATIONS[act][grade], ACTIVATIONS[gate][grade]
    length = np.full(B, T) if lens is None else np.asarray(lens).astype(np.int64)
    assert length.shape == (B,) and length.min() >= 1 and length.max() <= T
    dot = _product(bits)
    h = np.full((T, B, n), MARKER, dtype)
    out, cell = np.zeros((B, n), dtype), np.zeros((B, n), dtype)
    for s in range(int(length.max())):
        bb = np.nonzero(length > s)[0]                                # the chunks that have a step s
        t = length[bb] - 1 - s if reverse else np.full(len(bb), s)    # ... and where it lies in time
        v = vW[t, bb] if vW is not None else dot(x[t, bb], iW) + bias
        a = (v + dot(out[bb], sW)).reshape(len(bb), n, 4)
        c = cell[bb]
        cn = c * gatefun(a[:, :, 2] + c * peep[1])
        cn = cn + fun(a[:, :, 0]) * gatefun(a[:, :, 1] + c * peep[0])
        hn = fun(cn) * gatefun(a[:, :, 3] + cn * peep[2])
        assert hn.dtype == dtype and cn.dtype == dtype
        out[bb], cell[bb] = hn, cn
        h[t, bb] = hn
    return h


# ------------------------------------------------------------------------------------------------------------ inputs
REGIMES = ("moderate", "trained")


def weights(I, n, regime):
    """moderate: the distribution of tests/test_gpu_lstm_fused16.py's _params(scale=2.0).  trained: scale 3.0, sixty entries of
    -6 / 5 / 4.5 in sW, iW doubled."""
    rs = np.random.RandomState(1000 * I + n + (500 if regime == "trained" else 0))
    scale = 3.0 if regime == "trained" else 2.0
    iW = (rs.normal(size=(4 * n, I)) / np.sqrt(I + n)).astype(F32)
    sW = (scale * rs.normal(size=(4 * n, n)) / np.sqrt(2 * n)).astype(F32)
    b = rs.normal(size=4 * n).astype(F32)
    p = (rs.normal(size=(3, n)) / np.sqrt(n)).astype(F32)
    if regime == "trained":
        sW.reshape(-1)[rs.randint(0, sW.size, size=60)] = rs.choice([-6.0, 5.0, 4.5], size=60)
        iW *= F32(2.0)
    return iW, sW, b, p


class Case(dict):
    """Inputs, float64 reference `h` and yardstick result `hy` of one launch geometry.  `yard`: the largest error of the yardstick
    over the chunks of the case.  `take(B)` is the case of its first B chunks: chunks do not see each other, so the reference and the
    yardstick result of a smaller batch are slices, and its yardstick is taken over the chunks it has."""

    def __init__(self, **kw):
        super().__init__(**kw)
        if "yard" not in self:
            self["yard"] = float(chunk_errors(self["hy"], self["h"], self["lens"]).max())

    def take(self, B):
        if B == self["B"]:
            return self
        c = dict(self, B=B)
        del c["yard"]
        for k in ("x", "vW", "h", "hy"):
            if c.get(k) is not None:
                c[k] = np.ascontiguousarray(c[k][:, :B])
        if c["lens"] is not None:
            c["lens"] = c["lens"][:B]
        return Case(**c)


def summation_orders(I):
    """The orders in which the yardstick of a MIXED case sums its projection x.iW^T: as given, reversed, and two fixed shuffles; the
    yardstick is the worst of them.  Why only there, and why at all: the row of 1e3 times the rest makes gate inputs of order 1e3, sums
    of I terms of order 1e2 whose float32 partial sums are rounded at ulp(1e3) = 6e-5, so the sum is 1e-4 off whatever the operands'
    precision; of 4n such sums about one lands within +-1 of zero, where a gate passes its error on (times at most 1/4 .. 1): 1e-6 to
    1e-5 in h for that one chunk.  Its size depends on nothing but the order of the additions, which neither float32 nor
    include/sloika_amd.h fixes: over twelve orders of (60, 64), T = 7, forward, the same y22 arithmetic gives 2.9e-7 (the order as
    given) to 4.9e-6 for the chunk with that row and 2.4e-7 to 5.4e-7 for all others; lstm_fused16_kernel, which sums in the order of
    its MFMA blocks, was 1.5e-6 from float64 there.  One order is one draw of that cost; elsewhere the sums are of order 1 to 10 and
    another order moves them by the ulps BOUND[0] is there for."""
    return [np.arange(I), np.arange(I)[::-1]] + [np.random.RandomState(seed).permutation(I) for seed in (1, 2)]


def _seed(I, n, T, lens):
    return 7 * I + 3 * n + T + (100 if lens is not None else 0)


@functools.lru_cache(maxsize=None)
def layer_case(I, n, regime, T, B, reverse, lens=None, mixed=False, bias=True, peep=True):
    """The case of slk_lstm_fused16_f32 at this geometry (yardstick y22, both products rounded): made once, shared by every test
    that asks, and left unchanged.  bias / peep False: the forms with b = NULL / p = NULL."""
    iW, sW, b, p = weights(I, n, regime)
    b, p = (b if bias else None), (p if peep else None)
    x = inputs(I, T, B, _seed(I, n, T, lens), mixed)
    ln = None if lens is None else np.asarray(lens, np.int32)
    h = lstm_forward(x, iW, sW, b, p, reverse, ln)
    hy = [lstm_forward(np.ascontiguousarray(x[:, :, k]), np.ascontiguousarray(iW[:, k]), sW, b, p, reverse, ln, F32, 22)
          for k in (summation_orders(I) if mixed else [np.arange(I)])]
    hy = max(hy, key=lambda v: chunk_errors(v, h, ln).max())
    return Case(I=I, n=n, regime=regime, T=T, B=B, reverse=reverse, lens=ln, x=x, vW=None, iW=iW, sW=sW, b=b, p=p, act="tanh",
                gate="sigmoid", grade="y22", h=h, hy=hy)


SCAN_INSIZE = 24                    # the projection of the scan cases is made here, in float64; any input width will do


@functools.lru_cache(maxsize=None)
def scan_case(n, T, B, reverse, lens=None, peep=True, grade="y22", acts=("tanh", "sigmoid")):
    """The case of the scan entries: vW is the float32 rounding of the float64 projection.  grade y22 (slk_lstm_scan16_f32) rounds
    the operands of the recurrent product; y32 (slk_lstm_recurrent*_f32) is plain float32."""
    I = SCAN_INSIZE
    iW, sW, b, p = weights(I, n, "moderate")
    p = p if peep else None
    x = inputs(I, T, B, _seed(I, n, T, lens))
    ln = None if lens is None else np.asarray(lens, np.int32)
    vW = (x.astype(F64) @ iW.astype(F64).T + b.astype(F64)).astype(F32)
    act, gate = acts
    return Case(I=I, n=n, regime="moderate", T=T, B=B, reverse=reverse, lens=ln, x=None, vW=vW, iW=None, sW=sW, b=None, p=p, act=act,
                gate=gate, grade=grade, h=lstm_forward(None, None, sW, None, p, reverse, ln, vW=vW, act=act, gate=gate),
                hy=lstm_forward(None, None, sW, None, p, reverse, ln, F32, {"y22": 22, "y32": None}[grade], vW=vW, act=act, gate=gate))


@functools.lru_cache(maxsize=None)
def gemm_case(I, n, T, B, reverse):
    """The case of slk_lstm_f32 (projection GEMM in float32 + float32 scan): yardstick y32 of the whole layer."""
    iW, sW, b, p = weights(I, n, "moderate")
    x = inputs(I, T, B, _seed(I, n, T, None))
    return Case(I=I, n=n, regime="moderate", T=T, B=B, reverse=reverse, lens=None, x=x, vW=None, iW=iW, sW=sW, b=b, p=p, act="tanh",
                gate="sigmoid", grade="y32", h=lstm_forward(x, iW, sW, b, p, reverse), hy=lstm_forward(x, iW, sW, b, p, reverse, None, F32))


# ------------------------------------------------------------------------------------------------------- case tables
#: slk_lstm_fused16_f32: lstm_fused16_kernel<1> for insize up to 32, <2> above; n = 16, 32, 48 run with dead units
FUSED_SHAPES = [(12, 64), (64, 64), (4, 16), (36, 48), (32, 32), (60, 64)]
#: slk_lstm_scan16_f32: lstm_scan16_kernel<64> for n up to 64, <128> above
SCAN_SIZES = [16, 32, 48, 64, 80, 96, 112, 128]
#: slk_lstm_recurrent*_f32: lstm_mfma_kernel at these, lstm_generic_kernel at those
MFMA_SIZES = [16, 32, 48, 64]
GENERIC_SIZES = [7, 20, 72, 136]
GEMM_SHAPES = [(12, 64), (5, 20)]
#: Time edges, B = 17: four full workgroups and a last one with one live chunk.  lstm_fused16_kernel steps in groups of four, has
#: group 0 projected and group 1 staged before the loop and requests group G + 2 at step 0 of group G (lstm_fused16.hip:222-243,
#: :257, :310-315); lstm_scan16_kernel keeps vW in four register sets and requests three steps ahead (lstm_scan16.hip:147, :173,
#: :230-235).  1 .. 9 holds every T % 4 and both sides of the first two group ends (4 | 5, 8 | 9); 12 | 13 and 16 | 17 the next two:
#: the first lengths at which a group requested in the loop is also used, and used from the register it was requested into.
EDGE_B = 17
EDGE_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17)
#: lstm_mfma_kernel stages vW in blocks of KB = 8 steps through a two-slot ring and flushes outputs a block late (lstm_mfma.hip:52,
#: :118-119, :125, :160-162): one and two steps; both sides of the ends of blocks 0, 1, 2 (7 | 8 | 9: the second slot and the first
#: late flush; 15 | 16 | 17: the first refill of slot 0; 23 | 24 | 25: of slot 1); 33: a refill that is also the last block.
MFMA_T = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33)
GENERIC_T = (1, 2, 9)
GENERIC_B = (1, 5)
BATCH_T = 9
BATCH_B = (1, 2, 3, 4, 5, 7, 8, 9)         # a last workgroup of one to three live chunks, the clamped staging row
LONG = (100, 33)                           # one run per kernel family, moderate
LONG_FUSED, LONG_SCAN, LONG_MFMA = (12, 64), 128, 64
#: `trained` and the mixed-magnitude x, asked for at these lengths.  A case runs where its y22 (these seeds, B = 17, the worse
#: direction) is at most TABLE_MARGIN * ADMIT: the yardstick is a float32 BLAS product, another host may sum it in another order, and a
#: case within a few per cent of the limit would be admitted on one machine and not on the next.  Where an asked length is not
#: admitted the table holds the longest admitted length of the same group of four steps below it (the same side of the same edge),
#: and nothing where there is none.  As measured where the tables were made (the limit is 2.25e-6), one entry is replaced; the comments
#: hold the largest y22 of the row, forward / reversed, and lengths next to the asked ones that would NOT be admitted, so that
#: nobody moves an entry there:
TABLE_MARGIN = 0.9
TRAINED_T_ASKED = (1, 4, 5, 8)
MIXED_T_ASKED = (7, 13)
EDGE_T_TRAINED = {
    (12, 64): (1, 4, 5, 8),      # T = 8: 4.96e-7 / 6.37e-7
    (64, 64): (1, 4, 5, 8),      # T = 8: 9.26e-7 / 1.57e-6 (T = 7: 1.66e-6 / 8.03e-7)
    (4, 16): (1, 4, 5, 8),       # T = 8: 1.16e-6 / 6.14e-7
    (36, 48): (1, 4, 5, 8),      # T = 8: 1.00e-6 / 4.36e-7
    (32, 32): (1, 4, 5, 8),      # T = 8: 1.25e-6 / 1.22e-6
    (60, 64): (1, 4, 5, 8),      # T = 5: 6.53e-7 / 8.88e-7;  T = 8: 6.22e-7 / 9.59e-7
}
EDGE_T_MIXED = {                 # (y22 of a mixed case: the worst of summation_orders())
    (12, 64): (7, 13),           # T = 13: 1.11e-6 / 1.30e-6.  Not admitted: T = 5: 2.28e-5 / 2.04e-5;  T = 12: 2.16e-6 / 2.57e-6
    (64, 64): (7, 13),           # T = 13: 4.09e-7 / 3.68e-7.  Not admitted: T = 5: 2.71e-5 / 2.22e-5;  T = 11: 1.14e-5 / 9.96e-6
    (4, 16): (7, 13),            # T = 13: 6.21e-7 / 4.43e-7.  Not admitted: T = 9: 4.33e-6 / 3.68e-6
    (36, 48): (7, 13),           # T = 13: 4.15e-7 / 5.01e-7.  Not admitted: T = 5: 1.75e-5 / 1.66e-5;  T = 12: 3.32e-6 / 7.36e-6
    (32, 32): (7, 13),           # T = 7: 4.26e-7 / 3.20e-7.   Not admitted: T = 9: 7.88e-6 / 3.25e-6
    (60, 64): (6, 13),           # T = 7: 3.09e-6 / 1.78e-6, replaced by T = 6: 4.91e-7 / 4.08e-7;  T = 13: 4.65e-7 / 5.66e-7
}

RAGGED_T, RAGGED_B = 17, 17
RAGGED_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17)
MFMA_RAGGED_T = 25
MFMA_RAGGED_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 24, 25)
GENERIC_LENS = (9, 1, 4, 5, 8)


def _walk(lengths):
    """B = 17.  Chunks 0 .. 15 walk through `lengths` (chunk b has entry b % len: every length once or twice, the second time in
    another slot of a four-chunk workgroup); chunk 16, which the last workgroup holds alone and whose rows its dead slots re-read,
    has length 1: everything behind its first row is NaN."""
    return tuple(lengths[b % len(lengths)] for b in range(RAGGED_B - 1)) + (1,)


def ragged_lens():
    return _walk(RAGGED_LENGTHS)


def mfma_ragged_lens():
    return _walk(MFMA_RAGGED_LENGTHS)


def edge_entries(I, n):
    """(regime, T, mixed) of the time-edge set of a fused shape."""
    return [("moderate", T, False) for T in EDGE_T] + [("trained", T, False) for T in EDGE_T_TRAINED[(I, n)]] + \
           [("moderate", T, True) for T in EDGE_T_MIXED[(I, n)]]


def listed_layer_cases():
    """Every argument tuple of layer_case the GPU tests run through slk_lstm_fused16_f32, batch sizes as the largest of their set."""
    out = []
    for I, n in FUSED_SHAPES:
        for reverse in (False, True):
            out += [(I, n, regime, T, EDGE_B, reverse, None, mixed) for regime, T, mixed in edge_entries(I, n)]
            out.append((I, n, "moderate", BATCH_T, max(BATCH_B), reverse))
            out.append((I, n, "moderate", RAGGED_T, RAGGED_B, reverse, ragged_lens()))
            out.append((I, n, "moderate", BATCH_T, EDGE_B, reverse, (BATCH_T,) * EDGE_B))
            out.append((I, n, "moderate", BATCH_T, EDGE_B, reverse, None, False, False, True))
            out.append((I, n, "moderate", BATCH_T, EDGE_B, reverse, None, False, True, False))
            out.append((I, n, "moderate", BATCH_T, EDGE_B, reverse, None, False, False, False))
    out.append(LONG_FUSED + ("moderate",) + LONG + (False,))
    return out


def listed_scan_cases():
    """Every argument tuple of scan_case the GPU tests run: slk_lstm_scan16_f32 (y22), then slk_lstm_recurrent*_f32 (y32)."""
    out = []
    for n in SCAN_SIZES:
        for reverse in (False, True):
            for peep in (True, False):
                out += [(n, T, EDGE_B, reverse, None, peep) for T in EDGE_T]
                out.append((n, BATCH_T, max(BATCH_B), reverse, None, peep))
                out.append((n, RAGGED_T, RAGGED_B, reverse, ragged_lens(), peep))
    out.append((LONG_SCAN,) + LONG + (False,))
    for n in MFMA_SIZES:
        for reverse in (False, True):
            out += [(n, T, EDGE_B, reverse, None, True, "y32") for T in MFMA_T]
            out.append((n, BATCH_T, max(BATCH_B), reverse, None, True, "y32"))
            out.append((n, MFMA_RAGGED_T, RAGGED_B, reverse, mfma_ragged_lens(), True, "y32"))
    out.append((LONG_MFMA,) + LONG + (False, None, True, "y32"))
    for n in GENERIC_SIZES:
        for reverse in (False, True):
            out += [(n, T, max(GENERIC_B), reverse, None, True, "y32") for T in GENERIC_T]
            out.append((n, max(GENERIC_T), max(GENERIC_B), reverse, GENERIC_LENS, True, "y32"))
    for n in GENERIC_SIZES + MFMA_SIZES:
        out.append((n, max(GENERIC_T), max(GENERIC_B), True, None, True, "y32", OTHER_PAIR))
    return out


# --------------------------------------------------------------------------------------------------- kernel geometry
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sloika_amd", "csrc")


def _one(pattern, src, name):
    found = re.findall(pattern, src)
    assert len(found) == 1, "%s: expected one match of %r, found %r" % (name, pattern, found)
    return found[0]


def declared_geometry():
    """The constants the edge tables are laid around, as the kernel sources state them:
    KB: steps per staged block of lstm_mfma_kernel;
    fused_group / scan_unroll: steps per turn of the step loop (`s += 4`) of lstm_fused16_kernel / lstm_scan16_kernel, each checked
    against the phases its body calls (`step(ic<k>{}, ...)`, k = 0 .. 3);
    fused_ahead: how many groups ahead lstm_fused16_kernel requests x; scan_sets, scan_ahead: the register sets of vW in
    lstm_scan16_kernel and how many steps ahead it requests."""
    src = {}
    for name in ("lstm_mfma.hip", "lstm_fused16.hip", "lstm_scan16.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            src[name] = fh.read()
    geo = {"KB": int(_one(r"constexpr int KB = (\d+);", src["lstm_mfma.hip"], "lstm_mfma.hip KB"))}
    for key, name in (("fused_group", "lstm_fused16.hip"), ("scan_unroll", "lstm_scan16.hip")):
        geo[key] = int(_one(r"for \(int s = 0; s < T; s \+= (\d+)\)", src[name], name + " step loop"))
        phases = re.findall(r"step\(ic<(\d+)>\{\}, s", src[name])
        assert [int(k) for k in phases] == list(range(geo[key])), "%s: the step loop advances by %d and calls phases %r" % (
            name, geo[key], phases)
    geo["fused_ahead"] = int(_one(r"xoff\(4 \* \(G \+ (\d+)\) \+ sj\)", src["lstm_fused16.hip"], "lstm_fused16.hip request"))
    geo["scan_sets"] = int(_one(r"f32x4 vs\[(\d+)\]\[NUP\];", src["lstm_scan16.hip"], "lstm_scan16.hip vs"))
    ahead, mask = _one(r"load_v\(vs\[\(ph \+ (\d+)\) & (\d+)\]\);", src["lstm_scan16.hip"], "lstm_scan16.hip request")
    assert int(mask) == geo["scan_sets"] - 1, "lstm_scan16.hip: %d register sets, index mask %s" % (geo["scan_sets"], mask)
    geo["scan_ahead"] = int(ahead)
    return geo


def demanded_edges(geo):
    """What the declared geometry asks of the tables: {table name: (lengths it must hold, the constant that says so)}."""
    g, ahead = geo["fused_group"], geo["fused_ahead"]
    fused = set(range(1, 2 * g + 2)) | {k * g + d for k in range(2, ahead + 3) for d in (0, 1)}
    sets = geo["scan_sets"]
    scan = set(range(1, 2 * sets + 2)) | {k * sets + d for k in (1, 2, 3, 4) for d in (0, 1)}
    kb = geo["KB"]
    mfma = {1, 2} | {k * kb + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {4 * kb + 1}
    return {"EDGE_T (fused16)": (fused, "the group of %d steps and the request %d groups ahead of lstm_fused16.hip" % (g, ahead)),
            "EDGE_T (scan16)": (scan, "the %d register sets of lstm_scan16.hip" % sets),
            "MFMA_T": (mfma, "KB = %d of lstm_mfma.hip" % kb)}


# ------------------------------------------------------------------------------------------------------- comparison
#: worst err / yardstick per kernel and largest yardstick per (grade, regime) over everything `check` has seen in this process
FIGURES = {"ratio": {}, "yard": {}}


def check(got, case, label="", kernel=None):
    """Per chunk, over that chunk's own steps: the largest absolute error of h against float64 is at most BOUND[0] * yard + BOUND[1],
    yard being the largest such error of the case's yardstick over the chunks of the case, and at most CAP.
    ratio = err / (yard + BOUND[1] / BOUND[0]): the bound is ratio <= BOUND[0]."""
    err = chunk_errors(got, case["h"], case["lens"])
    y = case["yard"]
    assert np.isfinite(y)
    bound = BOUND[0] * y + BOUND[1]
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    ratio = err[worst] / (y + BOUND[1] / BOUND[0])
    print("LSTMFWD %s err %.3e yardstick %s %.3e bound %.3e ratio %.2f chunk %d" % (label, err[worst], case["grade"], y, bound, ratio, worst))
    if kernel is not None:
        FIGURES["ratio"][kernel] = max(FIGURES["ratio"].get(kernel, 0.0), float(ratio) if np.isfinite(ratio) else np.inf)
        key = (case["grade"], case["regime"])
        FIGURES["yard"][key] = max(FIGURES["yard"].get(key, 0.0), y)
    failures = []
    if not (err <= bound).all():
        failures.append("%s: chunk %d is %.3e from the float64 recursion, the yardstick %.3e allows %.3e" % (label, worst, err[worst], y, bound))
    if not (err <= CAP).all():
        failures.append("%s: chunk %d is %.3e from the float64 recursion, beyond the suite's %.1e" % (label, worst, err[worst], CAP))
    assert not failures, "\n".join(failures)
