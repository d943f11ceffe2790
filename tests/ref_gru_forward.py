"""Plain-numpy restatement of the forward Gru layer (sloika/layers.py:1010-1021, h(-1) = 0; Reverse: layers.py:1449-1450), written
from the formulas as a loop of its own, for tests/test_gpu_gru_forward_edges.py and tests/test_ref_gru_forward.py.

Three grades of the same recursion, as in tests/ref_reverse_scans.py (whose `round22`, `BOUND` and `sigmoid` are used here):
  * float64 (`gru_forward`): THE reference.  Pinned on the CPU to oracle_np.gru and to the C oracle (tests/test_ref_gru_forward.py).
  * `y32`: dtype=float32.  What float32 alone costs: the yardstick of the float32 scan of csrc/recurrent.hip (gru_mfma_kernel,
    gru_generic_kernel) behind slk_gru_recurrent*_f32 and the fallback of slk_gru_f32.
  * `y22`: float32 with both operands of the three products x.iW^T, h.sW^T and (r*h).sW2^T rounded to the 22 significand bits of an
    fp16 hi + lo pair (a row of x, h or r*h is one operand vector, a weight row one output unit's weights) -- the precision
    include/sloika_amd.h promises for the whole-layer kernels, not their code.
The yardsticks' distance from float64 is what a kernel of that arithmetic may cost, times `BOUND`.

Ragged batches: with `lens`, chunk b runs over its own lens[b] steps, a reversed scan starts at that chunk's own last step, and
entries at t >= lens[b] come back as MARKER.  Also here: the case generators (fixed seeds), the tables of cases the GPU tests run, and
`check`, the one comparison every GPU test of the forward Gru goes through."""
import functools
import re
import os

import numpy as np

from tests.ref_reverse_scans import BOUND, round22, sigmoid

F32, F64 = np.float32, np.float64
MARKER = np.nan
#: what the suite already demands of the forward kernels (tests/test_gpu_gru_bar16.py: err < 2e-5 against the C oracle)
CAP = 2e-5
#: a case is admitted where its yardstick (y22; y32 for the float32 scan) is at most this: BOUND then sits well inside CAP and the cap never decides
ADMIT = CAP / 8

SHAPES = [(96, 96), (64, 64), (32, 96), (128, 96), (64, 96), (48, 32), (16, 64)]
SCAN_SIZES = [112, 128, 144]
SCAN_INSIZE = 48                    # the projection of the wide-scan cases is made here, in float64; any input width will do


# ------------------------------------------------------------------------------------------------------- the recursion
def _chain(v, W):
    """v[B][K] . W[N][K]^T in float32 with ONE accumulator per sum, the terms added in the order of k."""
    return np.add.accumulate(v[:, None, :] * W[None, :, :], axis=2, dtype=F32)[:, :, -1]


def _product(bits, order=None):
    """v[B][K] . W[N][K]^T: as the operands are (order "chain": float32, summed as `_chain` does), or with both at 22 bits."""
    if order == "chain":
        assert bits is None
        return _chain
    if bits is None:
        return lambda v, W: v @ W.T
    assert bits == 22
    return lambda v, W: round22(v, 1) @ round22(W, 1).T


def _retu(x):
    return np.tanh(np.maximum(x, x.dtype.type(0)))                                      # SLK_ACT_RETU: tanh(max(x, 0))


def _sigmoid_pm(x):
    return np.clip(x.dtype.type(0.5) + x.dtype.type(0.25) * x, x.dtype.type(0), x.dtype.type(1))    # SLK_ACT_SIGMOID_PM


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, x.dtype.type(0))))                 # SLK_ACT_ELU: x, or exp(x) - 1 below zero


#: name -> (the function, in the dtype it is handed; its id in include/sloika_amd.h): restatements of slk_act (csrc/common.h) for the
#: pairs the float32 scan is run with
ACTIVATIONS = {"linear": (lambda x: x, 0), "tanh": (np.tanh, 1), "sigmoid": (sigmoid, 2), "elu": (_elu, 3), "retu": (_retu, 11),
               "sigmoid_pm": (_sigmoid_pm, 13)}
OTHER_PAIRS = (("retu", "sigmoid_pm"), ("linear", "sigmoid"), ("elu", "sigmoid"))


def gru_forward(x, iW, sW, sW2, b, reverse, lens=None, dtype=F64, bits=None, vI=None, act="tanh", gate="sigmoid", order=None):
    """x:[T][B][I] (time order), iW:[3n][I], sW:[2n][n], sW2:[n][n], b:[3n] or None -> (h:[T][B][n], zr:[T][B][2n] = z | r).
    vI:[T][B][3n], when given, stands for x.iW^T + b (the wide layers' scan takes the projection from a GEMM) and x, iW, b are not read.
    Per scan step (layers.py:1010-1021):  vI = x iW^T + b;  vS = h sW^T;  z = sig(vI[:n] + vS[:n]);  r = sig(vI[n:2n] + vS[n:]);
    c = tanh(vI[2n:] + (r h) sW2^T);  h' = z h + (1 - z) c.  act / gate: other names of ACTIVATIONS in the place of tanh / sig."""
    fun, gatefun = ACTIVATIONS[act][0], ACTIVATIONS[gate][0]
    sW, sW2 = np.asarray(sW, dtype), np.asarray(sW2, dtype)
    n = sW2.shape[0]
    if vI is None:
        x, iW = np.asarray(x, dtype), np.asarray(iW, dtype)
        bias = np.zeros(3 * n, dtype) if b is None else np.asarray(b, dtype)
        T, B = x.shape[:2]
    else:
        vI = np.asarray(vI, dtype)
        T, B = vI.shape[:2]
    length = np.full(B, T) if lens is None else np.asarray(lens).astype(np.int64)
    assert length.shape == (B,) and length.min() >= 1 and length.max() <= T
    assert order is None or dtype == F32
    dot, one = _product(bits, order), dtype(1)
    h = np.full((T, B, n), MARKER, dtype)
    zr = np.full((T, B, 2 * n), MARKER, dtype)
    state = np.zeros((B, n), dtype)
    for s in range(int(length.max())):
        bb = np.nonzero(length > s)[0]                                # the chunks that have a step s
        t = length[bb] - 1 - s if reverse else np.full(len(bb), s)    # ... and where it lies in time
        v = vI[t, bb] if vI is not None else dot(x[t, bb], iW) + bias
        hp = state[bb]
        vS = dot(hp, sW)
        z, r = gatefun(v[:, :n] + vS[:, :n]), gatefun(v[:, n:2 * n] + vS[:, n:])
        c = fun(v[:, 2 * n:] + dot(r * hp, sW2))
        hn = z * hp + (one - z) * c
        state[bb] = hn
        h[t, bb], zr[t, bb] = hn, np.concatenate([z, r], axis=1)
    assert h.dtype == dtype and zr.dtype == dtype
    return h, zr


def gru_stack(x, layers, lens=None, dtype=F64, bits=None):
    """Layers of n -> n, directions alternating and starting reversed, each fed the one before: the last layer's h.  Every layer is
    evaluated over a chunk's own steps: a forward layer's own rows do not depend on what lies behind them."""
    cur = x
    for k, (iW, sW, sW2, b) in enumerate(layers):
        cur = gru_forward(cur, iW, sW, sW2, b, bool((k + 1) & 1), lens, dtype, bits)[0]
    return cur


# ------------------------------------------------------------------------------------------------------------ inputs
REGIMES = ("moderate", "trained")


def weights(I, n, regime):
    """moderate: the distribution of tests/test_gpu_gru_bar16.py's _params(scale=2.0).  trained: scale 3.0, sixty entries of
    -6 / 5 / 4.5 in sW and in sW2, iW doubled (test_bar16_trained_weight_magnitudes)."""
    rs = np.random.RandomState(1000 * I + n + (500 if regime == "trained" else 0))
    scale = 3.0 if regime == "trained" else 2.0
    iW = (rs.normal(size=(3 * n, I)) / np.sqrt(I + n)).astype(F32)
    sW = (scale * rs.normal(size=(2 * n, n)) / np.sqrt(2 * n)).astype(F32)
    sW2 = (scale * rs.normal(size=(n, n)) / np.sqrt(2 * n)).astype(F32)
    b = rs.normal(size=3 * n).astype(F32)
    if regime == "trained":
        for m in (sW, sW2):
            m.reshape(-1)[rs.randint(0, m.size, size=60)] = rs.choice([-6.0, 5.0, 4.5], size=60)
        iW *= F32(2.0)
    return iW, sW, sW2, b


def inputs(I, T, B, seed, mixed=False):
    """Standard-normal x:[T][B][I].  mixed: inside the second group of four steps (the first where T < 8) chunk 1's row of one step is
    1e-3 times and chunk 2's row of the next step 1e3 times the rest (chunk 0 where the batch is smaller)."""
    x = np.random.RandomState(seed).normal(size=(T, B, I)).astype(F32)
    if mixed:
        t0 = 4 if T >= 8 else 0
        x[min(t0 + 1, T - 1), min(1, B - 1)] *= F32(1e-3)
        x[min(t0 + 2, T - 1), min(2, B - 1)] *= F32(1e3)
    return x


class Case(dict):
    """Inputs, float64 reference and yardstick of one launch geometry.  `grade` names the yardstick: "y22" (the default; its result is
    in h22 / zr22) or "y32" (h32).  `yard`: the largest error of the yardstick's result over the
    chunks of the case, for h and for z | r.  `take(B)` is the case of its first B chunks: chunks do not see each other, so the
    reference and the y22 result of a smaller batch are slices, and its yardstick is taken over the chunks it has."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.setdefault("grade", "y22")
        if "yard" not in self:
            sfx = {"y22": "22", "y32": "32"}[self["grade"]]
            self["yard"] = {k: float(chunk_errors(self[k + sfx], self[k], self["lens"]).max()) for k in ("h", "zr")
                            if self.get(k) is not None}

    def take(self, B):
        if B == self["B"]:
            return self
        c = dict(self, B=B)
        del c["yard"]
        for k in ("x", "vI", "h", "zr", "h22", "zr22", "h32"):
            if c.get(k) is not None:
                c[k] = np.ascontiguousarray(c[k][:, :B])
        if c["lens"] is not None:
            c["lens"] = c["lens"][:B]
        return Case(**c)


@functools.lru_cache(maxsize=None)
def layer_case(I, n, regime, T, B, reverse, lens=None, mixed=False):
    """The case of slk_gru_bar16_f32 at this geometry: made once, shared by every plan and test that asks, and left unchanged."""
    iW, sW, sW2, b = weights(I, n, regime)
    x = inputs(I, T, B, 7 * I + 3 * n + T + (100 if lens is not None else 0), mixed)
    ln = None if lens is None else np.asarray(lens, np.int32)
    h, zr = gru_forward(x, iW, sW, sW2, b, reverse, ln)
    h22, zr22 = gru_forward(x, iW, sW, sW2, b, reverse, ln, F32, 22)
    return Case(I=I, n=n, regime=regime, T=T, B=B, reverse=reverse, lens=ln, x=x, vI=None, iW=iW, sW=sW, sW2=sW2, b=b,
                h=h, zr=zr, h22=h22, zr22=zr22, cap=CAP)


@functools.lru_cache(maxsize=None)
def scan_case(n, T, B, reverse, lens=None):
    """The case of slk_gru_scan16_f32: vI is the float32 rounding of the float64 projection, and y22 rounds the operands of the two
    recurrent products only."""
    I = SCAN_INSIZE
    iW, sW, sW2, b = weights(I, n, "moderate")
    x = inputs(I, T, B, 7 * I + 3 * n + T + (100 if lens is not None else 0))
    ln = None if lens is None else np.asarray(lens, np.int32)
    vI = (x.astype(F64) @ iW.astype(F64).T + b.astype(F64)).astype(F32)
    h, zr = gru_forward(None, None, sW, sW2, None, reverse, ln, vI=vI)
    h22, zr22 = gru_forward(None, None, sW, sW2, None, reverse, ln, F32, 22, vI=vI)
    return Case(I=I, n=n, regime="moderate", T=T, B=B, reverse=reverse, lens=ln, x=None, vI=vI, iW=None, sW=sW, sW2=sW2, b=None,
                h=h, zr=zr, h22=h22, zr22=zr22, cap=CAP)


#: the recurrent weights of f32_scan_case are those of `weights(..., "moderate")` times this.  1.0: every entry of the time-edge, batch-edge
#: and ragged sets is admitted as it is (the largest y32 among them is in the comment beside F32_T), so nothing was lowered.
F32_RECURRENT_SCALE = 1.0
#: The orders in which the y32 yardstick of the float32 scan sums its products; the yardstick is the worse of them.  None: as the
#: host's BLAS does (blocked, several partial sums); "chain": one accumulator, the terms in the order of k -- the plainest float32
#: loop there is.  Neither float32 nor include/sloika_amd.h fixes the order, and a chain of n terms rounds n times at the size of its
#: partial sums where blocked sums round a few times: at n = 64 .. 144 the chain is 1.2 to 2.2 times further from float64 than BLAS
#: (the same at n = 16), most where the candidate is not squashed (linear, elu) and the sums are of order ten.  One order is one draw
#: of that cost.  What showed it: gru_generic_kernel, which sums in one fmaf chain, was 1.53e-6 from float64 at n = 144, elu / sigmoid,
#: T = 4, where the BLAS-order recursion is 3.2e-7 (ratio 4.03) and the chain-order recursion 5.2e-7.
F32_ORDERS = (None, "chain")


@functools.lru_cache(maxsize=None)
def f32_scan_case(n, T, B, reverse, lens=None, act="tanh", gate="sigmoid"):
    """The case of slk_gru_recurrent_f32 / _ex / _ragged_f32 (csrc/recurrent.hip): as scan_case, moderate weights and vI the float32
    rounding of the float64 projection; the float64 recursion and the y32 yardstick both run over that vI."""
    I = SCAN_INSIZE
    iW, sW, sW2, b = weights(I, n, "moderate")
    sW, sW2 = (sW * F32(F32_RECURRENT_SCALE)).astype(F32), (sW2 * F32(F32_RECURRENT_SCALE)).astype(F32)
    x = inputs(I, T, B, 7 * I + 3 * n + T + (100 if lens is not None else 0))
    ln = None if lens is None else np.asarray(lens, np.int32)
    vI = (x.astype(F64) @ iW.astype(F64).T + b.astype(F64)).astype(F32)
    h = gru_forward(None, None, sW, sW2, None, reverse, ln, vI=vI, act=act, gate=gate)[0]
    h32 = [gru_forward(None, None, sW, sW2, None, reverse, ln, F32, None, vI=vI, act=act, gate=gate, order=o)[0] for o in F32_ORDERS]
    h32 = max(h32, key=lambda v: chunk_errors(v, h, ln).max())
    return Case(I=I, n=n, regime="moderate", T=T, B=B, reverse=reverse, lens=ln, x=None, vI=vI, iW=None, sW=sW, sW2=sW2, b=None,
                act=act, gate=gate, grade="y32", h=h, zr=None, h32=h32, cap=CAP)


@functools.lru_cache(maxsize=None)
def f32_layer_case(I, n, T, B, reverse, lens=None, grade="y32", act="tanh", gate="sigmoid", seed=0):
    """The case of a whole layer whose recurrence is the float32 scan (slk_gru_f32's GEMM + scan fallback; layers.Gru on the "scan"
    plan): float64 from x, and the yardstick of the whole layer, projection included -- y32 where the projection is a float32 GEMM,
    y22 where it is the fp16 split."""
    iW, sW, sW2, b = weights(I, n, "moderate")
    x = inputs(I, T, B, 7 * I + 3 * n + T + seed + (100 if lens is not None else 0))
    ln = None if lens is None else np.asarray(lens, np.int32)
    h = gru_forward(x, iW, sW, sW2, b, reverse, ln, act=act, gate=gate)[0]
    hy = [gru_forward(x, iW, sW, sW2, b, reverse, ln, F32, {"y32": None, "y22": 22}[grade], act=act, gate=gate, order=o)[0]
          for o in (F32_ORDERS if grade == "y32" else (None,))]
    hy = max(hy, key=lambda v: chunk_errors(v, h, ln).max())
    return Case(I=I, n=n, regime="moderate", T=T, B=B, reverse=reverse, lens=ln, x=x, vI=None, iW=iW, sW=sW, sW2=sW2, b=b,
                act=act, gate=gate, grade=grade, h=h, zr=None, cap=CAP, **{"h" + grade[1:]: hy})


def stack_weights(n, nlayer):
    """Layer k of an n -> n stack: the moderate distribution, a seed per layer."""
    out = []
    for k in range(nlayer):
        rs = np.random.RandomState(4000 + 10 * n + k)
        out.append(((rs.normal(size=(3 * n, n)) / np.sqrt(2 * n)).astype(F32), (2.0 * rs.normal(size=(2 * n, n)) / np.sqrt(2 * n)).astype(F32),
                    (2.0 * rs.normal(size=(n, n)) / np.sqrt(2 * n)).astype(F32), rs.normal(size=3 * n).astype(F32)))
    return out


STACK_T, STACK_B = 9, 5
STACK_LENS = (9, 1, 4, 5, 8)          # a chunk of length 1, a full one, both sides of a group of four, one short of the ring
STACK_LAYERS = (1, 2, 5)
STACK_SIZES = (96, 64)


@functools.lru_cache(maxsize=None)
def stack_case(n, nlayer):
    """slk_gru_bar16_stack_f32: the float64 stack and the y22 stack of the same layers; the cap is the layer's times nlayer."""
    T, B = STACK_T, STACK_B
    layers = stack_weights(n, nlayer)
    x = inputs(n, T, B, 31 * n + nlayer)
    ln = np.asarray(STACK_LENS, np.int32)
    return Case(I=n, n=n, regime="moderate", T=T, B=B, reverse=None, lens=ln, x=x, vI=None, layers=layers, h=gru_stack(x, layers, ln),
                zr=None, h22=gru_stack(x, layers, ln, F32, 22), zr22=None, cap=CAP * nlayer)


# ------------------------------------------------------------------------------------------------------- case tables
#: the plans of slk_gru_bar16_f32 (bits 8-9 of `reverse`) -> kernel file, chunks per workgroup
PLANS = {1: ("gru_bar16_body.h", 4), 2: ("gru_bar16d.hip", 8), 3: ("gru_bar16q.hip", 16)}
KERNEL = {1: "four", 2: "eight", 3: "sixteen"}
#: Time edges, B = 17 (every plan: full workgroups and a last one with one live chunk).  The four- and eight-chunk kernels project
#: in groups of GS = 4 steps into a ring of R = 8 (gru_bar16_body.h:18-19, gru_bar16d.hip:57-58), the sixteen-chunk kernel has
#: GS = 2, R = 4 (gru_bar16q.hip:46-47); x is requested three groups ahead (load_x(G + 3), gru_bar16_body.h:631).  1 .. 9 holds every
#: T % 4 and every T % 2, both sides of the first ring turnover (8 | 9; 4 | 5 for sixteen chunks); 12 | 13 the first prefetch that would
#: pass the end; 16 | 17 the second turnover.
EDGE_B = 17
EDGE_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17)
#: trained, asked for at T in {1, 4, 5, 8}: sixty weights of 4.5 .. 6 make the map expand, and any two evaluations drift apart with T.
#: A case runs where its y22 (these seeds, B = 17, h and z | r, the worse direction) is at most ADMIT = 2.5e-6, which
#: tests/test_ref_gru_forward.py asserts of every entry.  The tables keep a (shape, T) whose figure, as measured where they were made,
#: is at most TABLE_MARGIN * ADMIT: the yardstick is a float32 BLAS product, another host may sum it in another order, and a case
#: within a few per cent of the limit would be admitted on one machine and not on the next.  Taken out, with y22 forward / reversed:
TABLE_MARGIN = 0.9
TRAINED_T_ASKED = (1, 4, 5, 8)
EDGE_T_TRAINED = {
    (96, 96): (1,),              # T = 4: 2.47e-6 / 2.07e-6 (inside the margin);  T = 5: 3.07e-6 / 5.16e-6;  T = 8: 6.22e-6 / 7.22e-6
    (64, 64): (1,),              # T = 4: 2.27e-6 / 2.91e-6;  T = 5: 3.67e-6 / 1.76e-6;  T = 8: 4.61e-6 / 4.79e-6
    (32, 96): (1, 4),            # T = 5: 4.21e-6 / 2.36e-6;  T = 8: 3.10e-6 / 6.37e-6
    (128, 96): (1,),             # T = 4: 2.98e-6 / 3.33e-6;  T = 5: 2.89e-6 / 4.70e-6;  T = 8: 2.83e-6 / 6.87e-6
    (64, 96): (1, 4),            # T = 5: 8.63e-6 / 2.40e-6;  T = 8: 5.13e-6 / 5.58e-6
    (48, 32): (1,),              # T = 4: 4.26e-6 / 3.10e-6;  T = 5: 4.06e-6 / 7.07e-6;  T = 8: 2.09e-5 / 2.52e-5
    (16, 64): (1, 4),            # T = 5: 2.38e-6 / 2.32e-6 (inside the margin);  T = 8: 7.35e-6 / 1.15e-5
}
#: the x variant with rows 1e-3 and 1e3 times the rest inside one group of four steps (moderate weights), asked for at T in {7, 13}.
#: A row of 1e3 puts pre-activations of order 1e3 through float32: where one of them happens to land near zero, float32 itself is
#: 1e-5 off.  Same rule, taken out with the measured y22:
MIXED_T_ASKED = (7, 13)
EDGE_T_MIXED = {
    (96, 96): (7, 13),
    (64, 64): (7, 13),
    (32, 96): (7, 13),
    (128, 96): (7, 13),
    (64, 96): (),                # T = 7: 2.06e-5 / 2.10e-5;  T = 13: 2.98e-6 / 2.60e-6
    (48, 32): (7,),              # T = 13: 1.12e-5 / 1.14e-5
    (16, 64): (13,),             # T = 7: 4.39e-6 / 3.81e-6
}
SAVE_T = (1, 5, 9)
BATCH_T = 9
BATCH_B = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33)
SHARE_SHAPES = [(64, 64), (48, 32), (16, 64)]
SHARE_B = 9
AUTO_T = 2
#: wide scan: step s uses register set s % 4 and requests step s + 3 (gru_scan1t.hip:137-143 `VI vs[4]`, :171 `load_vi(vs[(ph + 3) & 3])`;
#: the step loop is unrolled by four, :243-248): 1 .. 9 has both sides of the first two periods (4 | 5, 8 | 9), 12 | 13 the third,
#: 16 | 17 the fourth.
SCAN_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17)

RAGGED_T, RAGGED_B = 17, 33
RAGGED_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17)


def ragged_lens():
    """T = 17, B = 33.  Chunks 0 .. 27 walk through RAGGED_LENGTHS (chunk b has entry b % 11: every length two or three times, in
    different slots of a four-, an eight- and a sixteen-chunk workgroup each time, 11 being odd); chunks 28 .. 31 are a four-chunk
    workgroup of length 1 only; chunk 32, the one every plan's last workgroup holds alone and its dead slots re-read, has length 1.
    (33 chunks cannot show each of eleven lengths to each of four slots, let alone sixteen: 44 > 33.  What holds is asserted in
    tests/test_ref_gru_forward.py.)"""
    lens = [RAGGED_LENGTHS[b % len(RAGGED_LENGTHS)] for b in range(28)] + [1] * 5
    assert len(lens) == RAGGED_B
    return tuple(lens)


def edge_entries(I, n):
    """(regime, T, mixed) of the time-edge set of a shape."""
    return [("moderate", T, False) for T in EDGE_T] + [("trained", T, False) for T in EDGE_T_TRAINED[(I, n)]] + \
           [("moderate", T, True) for T in EDGE_T_MIXED[(I, n)]]


def listed_layer_cases():
    """Every (I, n, regime, T, B, reverse, lens, mixed) the GPU tests run through slk_gru_bar16_f32, batch sizes as the largest of
    their set (the smaller ones are its first chunks)."""
    out = []
    for I, n in SHAPES:
        for reverse in (False, True):
            out += [(I, n, regime, T, EDGE_B, reverse, None, mixed) for regime, T, mixed in edge_entries(I, n)]
            out.append((I, n, "moderate", BATCH_T, max(BATCH_B), reverse, None, False))
            out.append((I, n, "moderate", RAGGED_T, RAGGED_B, reverse, ragged_lens(), False))
            out.append((I, n, "moderate", BATCH_T, RAGGED_B, reverse, (BATCH_T,) * RAGGED_B, False))
    for I, n in SHAPES:
        if (I, n) in SHARE_SHAPES or (I, n) == (96, 96):
            for reverse in (False, True):
                out.append((I, n, "moderate", BATCH_T, SHARE_B, reverse, None, False))
                out.append((I, n, "moderate", BATCH_T, SHARE_B, reverse, share_lens(), False))
    return out


def share_lens():
    return (9, 1, 4, 5, 8, 2, 9, 3, 1)


def listed_scan_cases():
    out = []
    for n in SCAN_SIZES:
        for reverse in (False, True):
            out += [(n, T, EDGE_B, reverse, None) for T in SCAN_T]
            out.append((n, RAGGED_T, RAGGED_B, reverse, ragged_lens()))
    return out


# ------------------------------------------------------------------------- case tables of the float32 scan (csrc/recurrent.hip)
#: gru_mfma_kernel is instantiated for these (four K-slice layouts: SA / SB = 4 / 4 at 16 and 32, 2 / 4 at 48 and 64, 1 / 2 at 80 ..
#: 128 on four waves; N = 144 on twelve waves with two accumulators and `hold` re-read from LDS) ...
F32_MFMA_SIZES = (16, 32, 48, 64, 80, 96, 112, 128, 144)
#: ... and every other size takes gru_generic_kernel: below a wave, not a multiple of 4, between two instantiations, a multiple of 8
#: that is none of 16, and the first multiple of 16 past 144 (what layers.Gru hands over for anything wider)
F32_GENERIC_SIZES = (7, 20, 72, 136, 160)


def f32_kb(n):
    """Steps per staged block of gru_mfma_kernel<n> (`constexpr int KB = N <= 128 ? 8 : 4;`, tied to the source by
    declared_f32_scan_geometry and tests/test_ref_gru_forward.py)."""
    return 8 if n <= 128 else 4


#: Time edges by KB, at B = 17 (four full tiles of four chunks and a last one with one live chunk whose dead slots re-read it).  vI is
#: staged KB steps at a time into a two-slot ring, block k + 2 requested on the last step of block k, and h leaves one block late
#: through a second ring: one and two steps; both sides of the ends of blocks 0, 1, 2 (KB - 1 | KB | KB + 1: `if (T > KB)` and the
#: first late flush; 2 KB - 1 | 2 KB | 2 KB + 1: `s + 1 + KB < T`, the first refill of slot 0, whose request at T = 2 KB would pass the
#: end; 3 KB - 1 | 3 KB | 3 KB + 1: of slot 1); 4 KB + 1: a fourth block, and a refill that is also the last block.
#: Largest y32 (the worse of F32_ORDERS) over the time-edge, batch-edge and ragged sets as measured where the tables were made:
#: 9.26e-7 (n = 128, T = 16, reversed; per size 2.9e-7 at n = 16 to 9.3e-7 at n = 128); the limit is TABLE_MARGIN * ADMIT = 2.25e-6.
F32_T = {8: (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33), 4: (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 17)}
F32_EDGE_B = 17
#: at T = KB + 1 (both ring slots, a late flush and the tail flush): a last tile of one to three live chunks, one and two full tiles,
#: the clamped chunk index of the dead slots (`min(b0 + c, B - 1)`)
F32_BATCH_B = (1, 2, 3, 4, 5, 7, 8, 9)
#: ragged sets by KB: (T, the lengths): 1, both sides of the ends of blocks 0 and 1, 3 KB and T = 3 KB + 1
F32_RAGGED = {8: (25, (1, 7, 8, 9, 15, 16, 17, 24, 25)), 4: (13, (1, 3, 4, 5, 7, 8, 9, 12, 13))}
F32_RAGGED_B = 17
#: which entry of the lengths chunks 0 .. 11 have: three tiles of four chunks with four different lengths each -- the longest beside
#: the shortest in tile 0 (the DMA of a finished chunk is clamped to its last row while its neighbours go on), block-edge lengths
#: beside each other in tiles 1 and 2 -- and the three lengths that come twice (1, KB + 1, T) in another slot the second time
_F32_RAGGED_ORDER = (8, 0, 3, 5, 1, 7, 4, 2, 6, 3, 0, 8)
#: one long case per kernel form (four waves, twelve waves): T = 100 is 12 blocks and a tail of 4 at KB = 8, 25 blocks at KB = 4.
#: y32 as measured: see F32_LONG_T
F32_LONG_B = 6
F32_LONG_SIZES = (96, 144)
#: asked for at T = 100; n -> the T that runs.  y32 forward / reversed at T = 100: n = 96: 3.90e-7 / 5.49e-7;  n = 144: 7.74e-7 / 5.69e-7
#: (moderate weights contract: the yardstick does not grow with T), so neither is shortened
F32_LONG_T = {96: 100, 144: 100}
def f32_act_T(n):
    """T in (1, KB, KB + 1, 2 KB + 1) of the other-activation cases."""
    kb = f32_kb(n)
    return (1, kb, kb + 1, 2 * kb + 1)


#: other activations (the <N, -1, -1> instantiation; at n = 144 the portable kernel), B = 5
F32_ACT_SIZES = (16, 64, 96, 128)
F32_ACT_B = 5
F32_ACT_LENS = (9, 1, 4, 5, 8)
F32_GENERIC_T = (1, 2, 9)
F32_GENERIC_B = (1, 5)
F32_GENERIC_LENS = (9, 1, 4, 5, 8)
F32_FORCED_SIZES = (16, 96, 144)
#: (n, act) -> the lengths that run.  Asked for at f32_act_T(n); largest y32 per pair over the sizes, as measured: retu / sigmoid_pm
#: 2.74e-7, elu / sigmoid 1.60e-6 (n = 128, T = 17), linear / sigmoid 2.32e-6 (n = 128, T = 17: a candidate that is not squashed lets
#: the state grow, and float32's cost with it).  That one is past 2.25e-6 and runs at the largest admitted length below it instead:
#: T = 16: 2.59e-6;  T = 15: 2.09e-6.  (The next largest, linear at n = 144, T = 9 and n = 64, T = 17: 1.63e-6, 1.61e-6.)
F32_ACT_T = {(n, act): f32_act_T(n) for n in (16, 64, 96, 128, 144) for act, _ in OTHER_PAIRS}
F32_ACT_T[(128, "linear")] = (1, 8, 9, 15)
#: slk_gru_f32's fallback: (16, 16) has no whole-layer kernel; (40, 112) is too wide for one and its input no multiple of 16
F32_LAYER_SHAPES = ((16, 16), (40, 112))
F32_LAYER_TB = (9, 5)
#: layers.Gru on the "scan" plan, ragged inside a birnn (T, B and lengths of f32_ragged_lens(8)): wider than 144, which is the portable
#: kernel, and other activations at an MFMA size; the projection of both is the fp16 split (yardstick y22 of the whole layer) ...
F32_NET_SCAN = ((12, 160, "tanh", "sigmoid"), (12, 64, "retu", "sigmoid_pm"))
#: ... and a shape of the whole-layer kernel as SLOIKA_AMD_EXACT_F32=1 runs it: float32 GEMM + float32 scan (y32 of the whole layer)
F32_NET_EXACT = (96, 96)


def f32_ragged_lens(kb):
    """(T, lens) of the ragged set, B = 17: chunks 0 .. 11 take the lengths in _F32_RAGGED_ORDER, chunks 12 .. 15 are a tile of
    length 1 only, and chunk 16, which the last tile holds alone and whose rows its dead slots re-read, has length 1."""
    T, lengths = F32_RAGGED[kb]
    lens = tuple(lengths[k] for k in _F32_RAGGED_ORDER) + (1,) * 5
    assert len(lens) == F32_RAGGED_B
    return T, lens


def listed_f32_cases():
    """name of the set -> the argument tuples of f32_scan_case the GPU tests run (batch sizes as the largest of their set)."""
    out = {"edges": [], "long": [], "activations": [], "generic": []}
    for n in F32_MFMA_SIZES:
        kb = f32_kb(n)
        for reverse in (False, True):
            out["edges"] += [(n, T, F32_EDGE_B, reverse) for T in F32_T[kb]]
            out["edges"].append((n, kb + 1, max(F32_BATCH_B), reverse))
            T, lens = f32_ragged_lens(kb)
            out["edges"].append((n, T, F32_RAGGED_B, reverse, lens))
            out["edges"].append((n, T, F32_RAGGED_B, reverse, (T,) * F32_RAGGED_B))
    for n in F32_LONG_SIZES:
        out["long"] += [(n, F32_LONG_T[n], F32_LONG_B, reverse) for reverse in (False, True)]
    for n in F32_ACT_SIZES + (144,):
        for act, gate in OTHER_PAIRS:
            out["activations"] += [(n, T, F32_ACT_B, False, None, act, gate) for T in F32_ACT_T[(n, act)]]
            out["activations"].append((n, max(F32_ACT_LENS), F32_ACT_B, True, F32_ACT_LENS, act, gate))
    for n in F32_GENERIC_SIZES:
        for reverse in (False, True):
            out["generic"] += [(n, T, max(F32_GENERIC_B), reverse) for T in F32_GENERIC_T]
            out["generic"].append((n, max(F32_GENERIC_LENS), max(F32_GENERIC_B), reverse, F32_GENERIC_LENS))
    return out


# --------------------------------------------------------------------------------------------------- kernel geometry
CSRC =os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sloika_amd", "csrc")


def declared_geometry(plan):
    """(GS, whether R is declared as 2 * GS) as the plan's kernel source states them."""
    with open(os.path.join(CSRC, PLANS[plan][0])) as fh:
        src = fh.read()
    gs = re.findall(r"constexpr int GS = (\d+);", src)
    assert len(gs) == 1, (plan, gs)
    return int(gs[0]), len(re.findall(r"constexpr int R = 2 \* GS;", src)) == 1


def declared_scan_period():
    """(register sets of vI, steps the request runs ahead) as gru_scan1t.hip states them."""
    with open(os.path.join(CSRC, "gru_scan1t.hip")) as fh:
        src = fh.read()
    sets = re.findall(r"VI vs\[(\d+)\];", src)
    ahead = re.findall(r"load_vi\(vs\[\(ph \+ (\d+)\) & (\d+)\]\);", src)
    assert len(sets) == 1 and len(ahead) == 1, (sets, ahead)
    assert int(ahead[0][1]) == int(sets[0]) - 1
    return int(sets[0]), int(ahead[0][0])


def declared_f32_scan_geometry():
    """The constants the F32_* tables are laid around, as csrc/recurrent.hip states them: {"KB": (widest N of the first form, its KB,
    the KB above it), "tile": chunks per workgroup of gru_mfma_kernel}."""
    with open(os.path.join(CSRC, "recurrent.hip")) as fh:
        src = fh.read()
    kb = re.findall(r"constexpr int KB = N <= (\d+) \? (\d+) : (\d+);", src)
    tile = re.findall(r"const int b0 = blockIdx\.x \* (\d+);", src)
    grid = re.findall(r"dim3 grid\(\(B \+ (\d+)\) / (\d+)\)", src)
    assert len(kb) == 1 and len(tile) == 1 and len(grid) == 1, (kb, tile, grid)
    assert int(grid[0][1]) == int(tile[0]) == int(grid[0][0]) + 1, (tile, grid)
    return {"KB": tuple(int(v) for v in kb[0]), "tile": int(tile[0])}


def demanded_f32_edges(kb):
    """What a block of kb steps asks of a time-edge set: see the comment of F32_T."""
    return {1, 2} | {k * kb + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {4 * kb + 1}


# ------------------------------------------------------------------------------------------------------- comparison
#: worst err / yardstick per kernel and largest yardstick per grade and regime over everything `check` has seen in this process
FIGURES = {"ratio": {}, "y22": {}, "y32": {}}


def chunk_errors(got, ref, lens):
    """[B]: the largest |got - ref| over each chunk's own steps (NaN where `got` has one there)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    T, B = ref.shape[:2]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    length = np.full(B, T) if lens is None else np.asarray(lens)
    out = np.empty(B)
    for b in range(B):
        d = np.abs(got[:length[b], b] - ref[:length[b], b])
        out[b] = np.nan if np.isnan(d).any() else d.max()
    return out


def check(got_h, got_zr, case, label="", kernel=None):
    """Per chunk, over that chunk's own steps: the largest absolute error of h (and of z | r, where got_zr is given) against float64
    is at most BOUND[0] * y + BOUND[1], y being the largest such error of the case's yardstick (its `grade`: y22, or y32 for the
    float32 scan) over the chunks of the case, and at most the case's cap.  ratio = err / (y + BOUND[1] / BOUND[0]): the bound is
    ratio <= BOUND[0]."""
    grade = case.get("grade", "y22")
    lens = case["lens"]
    failures = []
    for what, got in (("h", got_h), ("zr", got_zr)):
        if got is None:
            continue
        err = chunk_errors(got, case[what], lens)
        y = case["yard"][what]
        assert np.isfinite(y)
        bound = BOUND[0] * y + BOUND[1]
        worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
        ratio = err[worst] / (y + BOUND[1] / BOUND[0])
        print("GRUFWD %s %s err %.3e yardstick %s %.3e bound %.3e ratio %.2f chunk %d" % (label, what, err[worst], grade, y, bound, ratio, worst))
        if kernel is not None:
            FIGURES["ratio"][kernel] = max(FIGURES["ratio"].get(kernel, 0.0), float(ratio) if np.isfinite(ratio) else np.inf)
            FIGURES[grade][case["regime"]] = max(FIGURES[grade].get(case["regime"], 0.0), y)
        if not (err <= bound).all():
            failures.append("%s %s: chunk %d is %.3e from the float64 recursion, the yardstick %.3e allows %.3e" % (
                label, what, worst, err[worst], y, bound))
        if not (err <= case["cap"]).all():
            failures.append("%s %s: chunk %d is %.3e from the float64 recursion, beyond the suite's %.1e" % (
                label, what, worst, err[worst], case["cap"]))
    assert not failures, "\n".join(failures)
