"""Plain-numpy restatements of the three sequential parts of a training step -- the Gru reverse scan, the Lstm cell recursion
and the Lstm reverse scan -- written from the formulas (layers.py:1010-1021, layers.py:677-697 and their hand-derived gradients as
sloika_amd/csrc/train.hip's comments state them), for tests/test_gpu_reverse_scans.py and tests/test_ref_reverse_scans.py.

Three grades of the same recursions:
  * float64 (`gru_reverse_scan`, `lstm_cell_scan`, `lstm_reverse_scan`): THE reference.  The Gru one takes the true candidate c.
    Pinned on the CPU to oracle_train.loss_and_grads (tests/test_ref_reverse_scans.py).
  * `y32`: the recursion in float32 arithmetic (`bits=None`); for the Gru with the candidate recovered from the layer output,
    c = clip((h_t - z h_prev) / (1 - z), -1, 1), 0 where 1 - z == 0, as any kernel that is handed h must.  What float32 alone costs.
  * `y22`: y32 with both operands of every matrix product rounded to the 22 significand bits of an fp16 hi + lo pair after a
    power-of-two scaling of the operand row to [1, 2) (`round22`) -- the precision include/sloika_amd.h promises for the fp16-split
    kernels, not their code.
The y32 / y22 results are yardsticks: their distance from the float64 reference, in the normalisation of `chunk_error`, is what a
kernel of that arithmetic may cost (times a small factor, see `BOUND`).

Rows are m = t*B + b in TIME order throughout; a reversed layer (reverse = 1) scans them from t = T-1 down to 0, so "the previous
scan step" of row t is row t+1.  Also here: the input generators (consistent forward passes in float64, rounded to float32 once)."""
import numpy as np

F32, F64 = np.float32, np.float64
REGIMES = ("moderate", "saturated", "trained", "mixed-1e-9", "mixed-1e+3")
#: Gru only: the saturated regime with the layer output h as a forward kernel leaves it, within H_NOISE of the float64 pass (the
#: forward kernels are held to 1e-4 of the oracle).  With h exact to float32 the recovered candidate is off by at most ulp(h) / (1 - z),
#: a few units where 1 - z is a few ulps, and enters the outputs times (1 - z): nothing shows, clamp or no clamp.  With h off by 1e-5
#: the quotient is off by hundreds there, and only the clamp to tanh's range keeps dac = g (1-z) (1-c^2) from being off by 1e-3 g.
#: The yardsticks recover the candidate from the same h (clamped, as documented), so what the noise legitimately costs is in them.
NOISY_H = "saturated-h1e-5"
H_NOISE = 1e-5


def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def _time(s, T, reverse):
    return T - 1 - s if reverse else s


def round22(a, axis):
    """Every vector along `axis` scaled by the power of two that brings its largest magnitude into [1, 2), cut into an fp16 hi half and
    an fp16 lo half of the remainder, and put together again: 22 significand bits, float32's exponent range."""
    a = np.asarray(a, F32).astype(F64)
    top = np.abs(a).max(axis=axis, keepdims=True)
    _, ex = np.frexp(np.where(top > 0, top, 1.0))                  # top = m 2^ex, m in [0.5, 1)
    sc = np.ldexp(1.0, 1 - ex)
    x = a * sc
    hi = x.astype(np.float16).astype(F64)
    lo = (x - hi).astype(np.float16).astype(F64)
    return ((hi + lo) / sc).astype(F32)


def _dot(bits):
    """The matrix product v[B][K] . W[K][N] of a scan step: float64 / float32 as the operands are, or with both operands at 22 bits
    (an operand row = one chunk's vector of the step; a weight row = the K weights of one output unit)."""
    if bits is None:
        return lambda v, W: v @ W
    assert bits == 22
    return lambda v, W: round22(v, 1) @ round22(W, 0)


# ---------------------------------------------------------------------------------------------------------------- Gru
def _gru_scan(dy, z, r, c, hp, sW, sW2, T, B, reverse, dot):
    """Reverse step, g = dL/dh_t + carry:  dac = g (1-z) (1-c^2);  daz = g (h-c) z (1-z);  drh = dac sW2;  dar = drh h r (1-r);
    carry = g z + drh r + [daz dar] sW.   sW:[2n][n], sW2:[n][n] as the layer stores them (vS = h sW^T)."""
    n = dy.shape[1]
    one = dy.dtype.type(1)
    da = np.zeros((T * B, 3 * n), dy.dtype)
    carry = np.zeros((B, n), dy.dtype)
    for s in range(T - 1, -1, -1):
        t = _time(s, T, reverse)
        m = slice(t * B, (t + 1) * B)
        g = dy[m] + carry
        dac = g * (one - z[m]) * (one - c[m] * c[m])
        daz = g * (hp[m] - c[m]) * z[m] * (one - z[m])
        drh = dot(dac, sW2)
        dar = drh * hp[m] * r[m] * (one - r[m])
        dzr = np.concatenate([daz, dar], axis=1)
        carry = g * z[m] + drh * r[m] + dot(dzr, sW)
        da[m] = np.concatenate([dzr, dac], axis=1)
    return da, r * hp


def gru_reverse_scan(dy, z, r, c, h_prev, sW, sW2, T, B, reverse):
    """float64.  dy, z, r, c, h_prev:[T*B][n] -> da:[T*B][3n] = [daz | dar | dac], rh:[T*B][n] = r * h_prev."""
    a = [np.asarray(v, F64) for v in (dy, z, r, c, h_prev, sW, sW2)]
    return _gru_scan(*a, T, B, bool(reverse), _dot(None))


def recovered_candidate(h, z, h_prev):
    """float32: c from h_t = z h_prev + (1 - z) c, clamped to tanh's range, 0 where 1 - z == 0."""
    h, z, h_prev = (np.asarray(v, F32) for v in (h, z, h_prev))
    omz = F32(1) - z
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.clip((h - z * h_prev) / omz, F32(-1), F32(1))
    return np.where(omz > 0, c, F32(0)).astype(F32)


def gru_reverse_scan_f32(dy, z, r, h, h_prev, sW, sW2, T, B, reverse, bits=None):
    """The yardsticks y32 (bits=None) and y22 (bits=22): float32 arithmetic, the candidate recovered from the layer output h."""
    a = [np.asarray(v, F32) for v in (dy, z, r, recovered_candidate(h, z, h_prev), h_prev, sW, sW2)]
    return _gru_scan(*a, T, B, bool(reverse), _dot(bits))


def product_f32(a, W, bits=None):
    """Yardstick of a separate product a[M][K] . W[K][N] (dL/dx = da . iW) in float32 / with 22-bit operands."""
    return _dot(bits)(np.asarray(a, F32), np.asarray(W, F32))


# --------------------------------------------------------------------------------------------------------------- Lstm
def _lstm_cells(sm, peep, T, B, reverse):
    """layers.py:677-697 given the summed gate inputs sm:[T*B][n][4] (candidate, input, forget, output), c_{-1} = 0:
    g = tanh(s0);  i = sig(s1 + c p0);  f = sig(s2 + c p1);  c' = c f + g i;  o = sig(s3 + c' p2)."""
    n = sm.shape[1]
    gates, cell = np.zeros_like(sm), np.zeros((T * B, n), sm.dtype)
    c = np.zeros((B, n), sm.dtype)
    for s in range(T):
        t = _time(s, T, reverse)
        m = slice(t * B, (t + 1) * B)
        g = np.tanh(sm[m, :, 0])
        i = sigmoid(sm[m, :, 1] + c * peep[0])
        f = sigmoid(sm[m, :, 2] + c * peep[1])
        c = c * f + g * i
        o = sigmoid(sm[m, :, 3] + c * peep[2])
        gates[m] = np.stack([g, i, f, o], axis=2)
        cell[m] = c
    return gates.reshape(T * B, 4 * n), cell


def _peep(peep, n, dtype):
    return np.zeros((3, n), dtype) if peep is None else np.asarray(peep, dtype).reshape(3, n)


def lstm_cell_scan(sum, peep, T, B, reverse, dtype=F64):
    """sum:[T*B][4n] interleaved j*4 + gate -> gates:[T*B][4n] (same layout, activated), cell:[T*B][n].  dtype=float32: the yardstick."""
    sm = np.asarray(sum, dtype)
    n = sm.shape[1] // 4
    return _lstm_cells(sm.reshape(T * B, n, 4), _peep(peep, n, dtype), T, B, bool(reverse))


def tanh_one_exp(x):
    """float32 tanh as the library documents its own (sloika_amd/csrc/common.h: "tanh through one exp: tanh(x) = 1 - 2/(exp(2x)+1); abs error
    < 3e-7 over the whole range"): accurate in ABSOLUTE terms, so 1 - tanh(c)^2 of a large cell state, itself a few 1e-7, is not
    accurate in relative terms the way numpy's correctly rounded float32 tanh leaves it."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) - F32(2) / (np.exp(F32(2) * x) + F32(1))).astype(F32)


def _lstm_scan(dy, gates, cell, sW, peep, T, B, reverse, dot, tanh=np.tanh):
    """With go = dL/dout_t + carry_out, tc = tanh(c_t):
    do' = go tc o(1-o);  dc = go o (1-tc^2) + do' p2 + carry_c;  di' = dc g i(1-i);  df' = dc c_{t-1} f(1-f);  dg' = dc i (1-g^2);
    carry_c = dc f + di' p0 + df' p1;  carry_out = [dg' di' df' do'] . sW;  dpeep[b] = sum_t (di' c_{t-1}, df' c_{t-1}, do' c_t)."""
    n = dy.shape[1]
    one = dy.dtype.type(1)
    gt = gates.reshape(T * B, n, 4)
    dsum = np.zeros((T * B, 4 * n), dy.dtype)
    dpeep = np.zeros((B, 3, n), dy.dtype)
    carry_out, carry_c = np.zeros((B, n), dy.dtype), np.zeros((B, n), dy.dtype)
    for s in range(T - 1, -1, -1):
        t = _time(s, T, reverse)
        m = slice(t * B, (t + 1) * B)
        if s > 0:
            tp = _time(s - 1, T, reverse)
            cp = cell[tp * B:(tp + 1) * B]
        else:
            cp = np.zeros((B, n), dy.dtype)                        # the scan starts from c = 0
        g, i, f, o = (gt[m, :, k] for k in range(4))
        go = dy[m] + carry_out
        tc = tanh(cell[m])
        do_ = go * tc * o * (one - o)
        dc = go * o * (one - tc * tc) + do_ * peep[2] + carry_c
        di = dc * g * i * (one - i)
        df = dc * cp * f * (one - f)
        dg = dc * i * (one - g * g)
        carry_c = dc * f + di * peep[0] + df * peep[1]
        d = np.stack([dg, di, df, do_], axis=2).reshape(B, 4 * n)
        carry_out = dot(d, sW)
        dsum[m] = d
        dpeep += np.stack([di * cp, df * cp, do_ * cell[m]], axis=1)
    return dsum, dpeep


def lstm_reverse_scan(dy, gates, cell, sW, peep, T, B, reverse, dtype=F64, bits=None):
    """dy:[T*B][n], gates:[T*B][4n], cell:[T*B][n], sW:[4n][n], peep:[3][n] or None -> dsum:[T*B][4n], dpeep:[B][3][n].
    float64 is the reference; dtype=float32 is y32, and with bits=22 y22.  The yardsticks take tanh(c_t) as `tanh_one_exp`: with
    numpy's own float32 tanh the saturated regime's y32 is 2.8e-7 for dpeep at n = 32, (T, B) = (3, 261), and 1.35e-6 with the
    documented formulation -- the loss sits in that one function, and it is the documented arithmetic, so it belongs in here."""
    a = [np.asarray(v, dtype) for v in (dy, gates, cell, sW)]
    return _lstm_scan(*a, _peep(peep, a[0].shape[1], dtype), T, B, bool(reverse), _dot(bits), np.tanh if dtype == F64 else tanh_one_exp)


# ----------------------------------------------------------------------------------------------- error normalisation
#: a kernel may cost BOUND[0] times its yardstick plus BOUND[1]: a different summation order and a hardware rcp / exp of one ulp in
#: place of numpy's; the additive term keeps a case whose yardstick happens to be ~0 (T = 1) from demanding exactness.
BOUND = (4.0, 4.0 * 2.0 ** -24)


def chunk_error(got, ref, T, B):
    """max over a chunk's T steps and columns of |got - ref|, divided by that chunk's largest |ref| (floor 1e-35): [B]."""
    g, w = np.asarray(got, F64).reshape(T, B, -1), np.asarray(ref, F64).reshape(T, B, -1)
    top = np.maximum(np.abs(w).max(axis=(0, 2)), 1e-35)
    return np.abs(g - w).max(axis=(0, 2)) / top


def chunk_abs_error(got, ref, T, B):
    g, w = np.asarray(got, F64).reshape(T, B, -1), np.asarray(ref, F64).reshape(T, B, -1)
    return np.abs(g - w).max(axis=(0, 2))


# ------------------------------------------------------------------------------------------------------------ inputs
def _preact(rs, shape, regime, gates=1):
    """Gate pre-activations [T][B][units * gates]: N(0, 2); saturated: N(0, 12) with one in fifty ten times that, so that float32
    sigmoids are exactly 1 (beyond +17.4) for several per cent and exactly 0 (beyond -104, which N(0, 12) alone never reaches) for
    some -- and, for cases of a few dozen elements, units 0, 1, 2 of the first scan step of chunk 0 at +40, -120 and +15 (float32
    sigmoid: 1, 0 and 1 - 3e-7) in every gate."""
    a = rs.normal(size=shape) * (12.0 if regime.startswith("saturated") else 2.0)
    if regime.startswith("saturated"):
        a[rs.uniform(size=shape) < 0.02] *= 10.0
        a[0, 0].reshape(-1, gates)[:3] = np.array([40.0, -120.0, 15.0])[:, None]
    return a


def _recurrent(rs, rows, n, regime):
    """[rows][n] recurrent weights; trained: the bulk at scale 3 with sixty entries of -6 / 5 / 4.5 (models/pretrained.pkl's sizes)."""
    w = (3.0 if regime == "trained" else 2.0) * rs.normal(size=(rows, n)) / np.sqrt(2 * n)
    if regime == "trained":
        w.reshape(-1)[rs.randint(0, w.size, size=60)] = rs.choice([-6.0, 5.0, 4.5], size=60)
    return w


def _dy(rs, T, B, n, regime):
    """dL/dh in scan order: every (step, chunk) at its own scale over three decades, three in ten exactly zero.  mixed-*: chunks
    b = 1 (mod 5) a million times smaller, b = 2 (mod 5) a thousand times larger, chunk 3 exactly zero, all times a global scale."""
    dy = rs.normal(size=(T, B, n)) * 10.0 ** rs.uniform(-3, 0, size=(T, B, 1))
    dy[rs.uniform(size=(T, B, n)) < 0.3] = 0.0
    if regime.startswith("mixed"):
        dy[:, 1::5] *= 1e-6
        dy[:, 2::5] *= 1e3
        dy[:, 3:4] = 0.0
        dy *= float(regime[len("mixed-"):])
    return dy


def assert_gru_saturated(case):
    """Regime 2 cannot silently go away: float32 update gates that ARE 1 and others within 1e-6 below it."""
    z = case["z"]
    assert z.dtype == F32 and (z == 1.0).any() and ((z > 1.0 - 1e-6) & (z < 1.0)).any()


def assert_lstm_saturated(case):
    """... and float32 forget and output gates that are exactly 0 and exactly 1."""
    gt = case["gates"]
    assert gt.dtype == F32
    for k in (2, 3):
        assert (gt[:, k::4] == 1.0).any() and (gt[:, k::4] == 0.0).any()


def _flip(a, reverse):
    return a[::-1] if reverse else a


def gru_case(seed, T, B, n, regime, reverse):
    """A consistent forward pass h_t = z h_{t-1} + (1 - z) c in float64, rounded to float32 once.  Arrays [T*B][.] in time order."""
    rs = np.random.RandomState(seed)
    z, r = sigmoid(_preact(rs, (T, B, n), regime)), sigmoid(_preact(rs, (T, B, n), regime))
    c = np.tanh(rs.normal(size=(T, B, n)) * 1.5)
    h = np.zeros((T + 1, B, n))
    for s in range(T):
        h[s + 1] = z[s] * h[s] + (1.0 - z[s]) * c[s]
    dy = _dy(rs, T, B, n, regime)
    if regime == NOISY_H:
        h[1:] = np.clip(h[1:] + rs.uniform(-H_NOISE, H_NOISE, size=(T, B, n)), -1.0, 1.0)
    out = {k: np.ascontiguousarray(_flip(v, reverse), dtype=F32).reshape(T * B, n)
           for k, v in dict(dy=dy, z=z, r=r, c=c, h=h[1:], h_prev=h[:-1]).items()}
    out["sW"], out["sW2"] = _recurrent(rs, 2 * n, n, regime).astype(F32), _recurrent(rs, n, n, regime).astype(F32)
    return out


def lstm_case(seed, T, B, n, regime, reverse, peepholes=True):
    """sum:[T*B][4n] float32; gates and cell = the float64 cell recursion of exactly those sums, rounded to float32 once."""
    rs = np.random.RandomState(seed)
    sm = np.ascontiguousarray(_flip(_preact(rs, (T, B, 4 * n), regime, 4), reverse), dtype=F32).reshape(T * B, 4 * n)
    peep = (rs.normal(size=(3, n)) / np.sqrt(n)).astype(F32)
    dy = np.ascontiguousarray(_flip(_dy(rs, T, B, n, regime), reverse), dtype=F32).reshape(T * B, n)
    sW = _recurrent(rs, 4 * n, n, regime).astype(F32)
    peep = peep if peepholes else None
    gates, cell = lstm_cell_scan(sm, peep, T, B, reverse)
    return dict(sum=sm, peep=peep, dy=dy, sW=sW, gates=gates.astype(F32), cell=cell.astype(F32))
