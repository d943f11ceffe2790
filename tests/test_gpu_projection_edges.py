"""The x-stationary projections at every K slab, tile, row and store edge, through the C ABI:
slk_linear_rowstats_f16x3 / slk_gemm_bias_act_f16x3 (csrc/gemm_rows_f16x3.hip), their weight split slk_split_f16x2_f32, and the
float32 twin slk_linear_rowstats_f32 (csrc/gemm_rows.hip).

Every launch writes into canaried buffers (tests/gpu_util.py) and reads x rows with NaN behind them; every check includes: guards
untouched, gaps between rows untouched, no NaN from an x gap in a result.  tests/projection_ref.py holds the reference arithmetic,
the shape lists and `paths`, the kernel's dispatch restated; tests/test_projection_ref.py asserts without a GPU that the lists
reach every path, and the tests here assert it again for the launches they make."""
import numpy as np
import pytest

from tests import projection_ref as pr
from tests.gpu_util import need_gpu, dev, stream, Out, padded_input, nan_filled, PATTERN

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ launch helpers
def _lead_buffer(a, ld, lead):
    """rows of `a` ld floats apart, the first one `lead` floats past a 16-byte boundary, NaN everywhere else -> (tensor, pointer)"""
    rows, w = a.shape
    if lead == 0:
        t = padded_input(a[:, None, :], None, ld)
    else:
        host = nan_filled(lead + rows * ld)
        host[lead:].reshape(rows, ld)[:, :w] = a
        t = dev(host)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * lead


class Weights:
    """W split on the device (the production path), and the bias"""

    def __init__(self, W, b):
        import torch
        from sloika_amd import _lib
        N, K = W.shape
        KP = pr.round_up(K, 16)
        self.N, self.K = N, K
        self.Wd = dev(W)
        self.hi = torch.empty((N, KP), dtype=torch.float16, device="cuda")
        self.lo = torch.empty((N, KP), dtype=torch.float16, device="cuda")
        self.inv = torch.empty((N,), dtype=torch.float32, device="cuda")
        assert _lib.lib().slk_split_f16x2_f32(self.Wd.data_ptr(), N, K, self.hi.data_ptr(), self.lo.data_ptr(), self.inv.data_ptr(),
                                              stream()) == 0
        self.b = None if b is None else dev(np.asarray(b, np.float32))

    def bptr(self):
        return None if self.b is None else self.b.data_ptr()


def run16(x, wt, lay, mode, what):
    """One launch of the fp16 kernel in `mode` ("stats": slk_linear_rowstats_f16x3 with statistics, else slk_gemm_bias_act_f16x3
    with that activation) -> (values [M][N], statistics [M][2] or None).  Guards and gaps are checked here."""
    from sloika_amd import _lib
    L = _lib.lib()
    M, K = x.shape
    N = wt.N
    xt, xp = _lead_buffer(x, lay.ldx(K), lay.x_lead)
    y = Out(M, 1, N, ld=lay.ldy(N), lead=lay.y_lead)
    if mode == "stats":
        st = Out(M, 1, 2)
        rc = L.slk_linear_rowstats_f16x3(xp, lay.ldx(K), wt.hi.data_ptr(), wt.lo.data_ptr(), wt.inv.data_ptr(), wt.bptr(), y.ptr(),
                                         lay.ldy(N), M, K, N, st.ptr(), stream())
    else:
        st = None
        rc = L.slk_gemm_bias_act_f16x3(xp, lay.ldx(K), wt.hi.data_ptr(), wt.lo.data_ptr(), wt.inv.data_ptr(), wt.bptr(), y.ptr(),
                                       lay.ldy(N), M, K, N, pr.ACTS[mode], stream())
    assert rc == 0, what
    y.fetch().assert_untouched_outside(None, "%s: y" % what)
    if st is not None:
        st.fetch().assert_untouched_outside(None, "%s: statistics" % what)
    del xt
    return y.values().reshape(M, N), None if st is None else st.values().reshape(M, 2)


def run32(x, W, b, lay, stats, w_lead, what):
    """One launch of slk_linear_rowstats_f32, W `w_lead` floats past a 16-byte boundary."""
    from sloika_amd import _lib
    M, K = x.shape
    N = W.shape[0]
    xt, xp = _lead_buffer(x, lay.ldx(K), lay.x_lead)
    wt, wp = _lead_buffer(W.reshape(1, -1), N * K, w_lead)
    bd = None if b is None else dev(np.asarray(b, np.float32))
    y = Out(M, 1, N, ld=lay.ldy(N), lead=lay.y_lead)
    st = Out(M, 1, 2) if stats else None
    rc = _lib.lib().slk_linear_rowstats_f32(xp, lay.ldx(K), wp, None if bd is None else bd.data_ptr(), y.ptr(), lay.ldy(N), M, K, N,
                                            st.ptr() if stats else None, stream())
    assert rc == 0, what
    y.fetch().assert_untouched_outside(None, "%s: y" % what)
    if stats:
        st.fetch().assert_untouched_outside(None, "%s: statistics" % what)
    del xt, wt
    return y.values().reshape(M, N), st.values().reshape(M, 2) if stats else None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ operands
def small_ints(rs, rows, K):
    """random integers in [-7, 7], at least one entry of magnitude 4 or more per row (no degenerate row scale)"""
    a = rs.randint(-7, 8, size=(rows, K))
    a[np.arange(rows), rs.randint(0, K, size=rows)] = rs.randint(4, 8, size=rows) * rs.choice([-1, 1], size=rows)
    return a.astype(np.float32)


_INT_CACHE = {}


def int_case(M, K, N):
    """x, W, b and the exact float32 logits with and without bias: computed once per shape, never modified"""
    key = (M, K, N)
    if key not in _INT_CACHE:
        rs = np.random.RandomState(1000003 * M + 1009 * K + N)
        x, W = small_ints(rs, M, K), small_ints(rs, N, K)
        b = rs.randint(-7, 8, size=N).astype(np.float32)
        dot = x.astype(np.int64) @ W.astype(np.int64).T
        assert np.abs(dot).max() + 7 < 2 ** 24
        case = (x, W, b, (dot + b.astype(np.int64)).astype(np.float32), dot.astype(np.float32))
        _INT_CACHE[key] = case
    return _INT_CACHE[key]


def real_case(M, K, N, seed=0):
    """the distribution of test_linear_rowstats_kernels_vs_float64: tanh(normal) x, weights at 1.5 sigma, one row times 4"""
    rs = np.random.RandomState(7919 * M + 131 * K + N + seed)
    x = np.tanh(rs.normal(size=(M, K))).astype(np.float32)
    W = (rs.normal(size=(N, K)) * 1.5).astype(np.float32)
    W[0, :] *= 4.0
    return x, W, rs.normal(size=N).astype(np.float32)


def check_stats(st, logits, what):
    """statistics against the device's own float32 logits: exact maximum, 1 / (1 / sum) to rtol 3e-6 (tests/test_gpu_gemm.py)"""
    m, s = pr.row_stats64(logits)
    np.testing.assert_array_equal(st[:, 0], m.astype(np.float32), err_msg=what)
    np.testing.assert_allclose(1.0 / st[:, 1].astype(np.float64), s, rtol=3e-6, err_msg=what)


def check_exact(out, st, want, mode, what):
    """`want`: the exact float32 pre-activation values"""
    assert np.isfinite(out).all(), what
    if mode in ("stats", "linear"):
        np.testing.assert_array_equal(bits(out), bits(want), err_msg=what)
    else:
        np.testing.assert_allclose(out, pr.act64(mode, want), rtol=2e-6, atol=2e-6, err_msg=what)
    if st is not None:
        check_stats(st, out, what)


def exact16(M, K, N, lay, mode="stats", bias=True):
    x, W, b, want_b, want_0 = int_case(M, K, N)
    what = "f16x3 %s M=%d K=%d N=%d %s%s" % (mode, M, K, N, lay, "" if bias else " no bias")
    out, st = run16(x, Weights(W, b if bias else None), lay, mode, what)
    check_exact(out, st, want_b if bias else want_0, mode, what)
    return out


def exact32(M, K, N, lay, w_lead, stats=True, bias=True):
    x, W, b, want_b, want_0 = int_case(M, K, N)
    what = "f32 M=%d K=%d N=%d %s w_lead=%d%s" % (M, K, N, lay, w_lead, "" if bias else " no bias")
    out, st = run32(x, W, b if bias else None, lay, stats, w_lead, what)
    check_exact(out, st, want_b if bias else want_0, "stats" if stats else "linear", what)
    return out


# ------------------------------------------------------------------------------------------------ a. exact on small integers
@pytest.mark.parametrize("lay", pr.LAYOUTS, ids=repr)
def test_f16x3_every_slab_exact_on_integers(lay):
    """Integers in [-7, 7]: the power-of-two scaling is exact, hi holds the integer and lo is 0, every product and partial sum is an
    integer below 2^24 -- so logits and row maximum must come out bit for bit in any summation order, for every KS = 1 .. 12, every
    lane-half mask of the last slab, both x loads, and (three layouts) every store path next to a ragged workgroup."""
    need_gpu()
    for K in pr.KS_SWEEP_K:
        p = lay.paths(pr.SWEEP_M, K, pr.SWEEP_N, stats=True)
        assert p["ks"] == (K + 15) // 16 and p["xload"] == ("vec16" if K % 8 == 0 and lay.x_lead == 0 else "elem")
        exact16(pr.SWEEP_M, K, pr.SWEEP_N, lay)


@pytest.mark.parametrize("K", pr.TILE_SWEEP_K)
def test_f16x3_every_tile_count_and_tail_exact(K):
    """1 to 7 tiles, 0 to 6 of them full: no second prefetch, odd and even passes of each wave half's two-tile loop, the leftover
    tile, the N % 4 == 0 partial-tile store and the dword tail; ring of 3 (K = 96) and of 2 (K = 176)."""
    need_gpu()
    seen = set()
    for N in pr.TILE_SWEEP_N:
        w = pr.ALIGNED.paths(pr.SWEEP_M, K, N, stats=True)["wgs"][0]
        seen.add((w["pairs"], w["handover"], w["tiles"][-1][1]))
        exact16(pr.SWEEP_M, K, N, pr.ALIGNED)
    assert {s[:2] for s in seen} == {(p, h) for p in (0, 1, 2) for h in ("none", "single")} | {(3, "none")}
    assert {s[2] for s in seen} == {"guard4", "tail4", "dword"}


@pytest.mark.parametrize("K,N", pr.ROW_SWEEP_KN)
def test_f16x3_every_row_edge_exact(K, N):
    need_gpu()
    for M in pr.ROW_SWEEP_M:
        exact16(M, K, N, pr.ALIGNED)
        exact16(M, K, N, pr.ODD_LDY)


@pytest.mark.parametrize("mode", pr.MODES)
def test_f16x3_every_instantiation_through_every_store(mode):
    """Each activation's kernel (and the statistics form) through the patch store, both float4 stores of the accumulators, the
    N % 4 == 0 tail and the dword store; with and without bias.  The pre-activation values are exact integers, so the activated
    output is held to the activation's own tolerance (test_all_activations_vs_oracle) and the linear one to equality."""
    need_gpu()
    stores = set()
    for (M, K, N) in pr.ACT_SHAPES:
        stores |= {c[3] for c in pr.combos(pr.mode_paths(pr.ALIGNED, M, K, N, mode))}
        exact16(M, K, N, pr.ALIGNED, mode)
        exact16(M, K, N, pr.ALIGNED, mode, bias=False)
    assert stores == set(pr.STORES)


@pytest.mark.parametrize("M,K,N", pr.ACT_SHAPES)
def test_f16x3_statistics_form_writes_the_same_logits(M, K, N):
    need_gpu()
    x, W, b = real_case(M, K, N)
    wt = Weights(W, b)
    for lay in (pr.ALIGNED, pr.ODD_LDY):
        with_st, st = run16(x, wt, lay, "stats", "stats form")
        without, _ = run16(x, wt, lay, "linear", "plain form")
        assert np.isfinite(with_st).all()
        np.testing.assert_array_equal(bits(with_st), bits(without))
        check_stats(st, with_st, "M=%d K=%d N=%d %s" % (M, K, N, lay))


def test_f16x3_lds_bias_limit():
    """N = 2047 and 2048 fill the staged bias and inverse-scale vectors to their last tile; one more column, or one more K, is
    refused with nothing written."""
    need_gpu()
    import torch
    from sloika_amd import _lib
    L = _lib.lib()
    for N in (2047, 2048):
        exact16(33, 16, N, pr.ALIGNED)
    x = dev(np.ones((33, 208), np.float32))
    for (K, N) in ((16, 2049), (193, 64)):
        KP = pr.round_up(K, 16)
        hi = torch.zeros((N, KP), dtype=torch.float16, device="cuda")
        inv = torch.ones((N,), dtype=torch.float32, device="cuda")
        y, st = Out(33, 1, N), Out(33, 1, 2)
        assert L.slk_linear_rowstats_f16x3(x.data_ptr(), 208, hi.data_ptr(), hi.data_ptr(), inv.data_ptr(), None, y.ptr(), N, 33, K, N,
                                           st.ptr(), stream()) == _lib.SLK_ERR_UNSUPPORTED
        assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), 208, hi.data_ptr(), hi.data_ptr(), inv.data_ptr(), None, y.ptr(), N, 33, K, N,
                                         1, stream()) == _lib.SLK_ERR_UNSUPPORTED
        assert (y.fetch().host == PATTERN).all() and (st.fetch().host == PATTERN).all()


def test_f16x3_argument_handling():
    need_gpu()
    import torch
    from sloika_amd import _lib
    L = _lib.lib()
    M, K, N = 5, 16, 8
    x = dev(np.ones((M, K), np.float32))
    hi = torch.zeros((N, K), dtype=torch.float16, device="cuda")
    inv = torch.ones((N,), dtype=torch.float32, device="cuda")
    y, st = Out(M, 1, N), Out(M, 1, 2)
    a = (hi.data_ptr(), hi.data_ptr(), inv.data_ptr(), None)
    assert L.slk_linear_rowstats_f16x3(x.data_ptr(), K, *a, y.ptr(), N, 0, K, N, st.ptr(), stream()) == 0          # M = 0
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K, *a, y.ptr(), N, 0, K, N, 1, stream()) == 0
    bad = _lib.SLK_ERR_INVALID_ARG
    assert L.slk_linear_rowstats_f16x3(x.data_ptr(), K - 1, *a, y.ptr(), N, M, K, N, st.ptr(), stream()) == bad    # ldx < K
    assert L.slk_linear_rowstats_f16x3(x.data_ptr(), K, *a, y.ptr(), N - 1, M, K, N, st.ptr(), stream()) == bad    # ldy < N
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K - 1, *a, y.ptr(), N, M, K, N, 1, stream()) == bad
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K, *a, y.ptr(), N - 1, M, K, N, 1, stream()) == bad
    # statistics belong to linear logits only: the kernel behind both entry points refuses them with an activation.  The C ABI
    # cannot express that pair (slk_gemm_bias_act_f16x3 has no statistics argument, slk_linear_rowstats_f16x3 no activation), so
    # what can be asked is asked: an activation outside the table is invalid, a valid one without an fp16 kernel unsupported
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K, *a, y.ptr(), N, M, K, N, -1, stream()) == bad
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K, *a, y.ptr(), N, M, K, N, 10 ** 6, stream()) == bad
    assert L.slk_gemm_bias_act_f16x3(x.data_ptr(), K, *a, y.ptr(), N, M, K, N, 7, stream()) == _lib.SLK_ERR_UNSUPPORTED
    assert (y.fetch().host == PATTERN).all() and (st.fetch().host == PATTERN).all()
    # the float32 twin
    W = dev(np.ones((N, K), np.float32))
    assert L.slk_linear_rowstats_f32(x.data_ptr(), K, W.data_ptr(), None, y.ptr(), N, 0, K, N, st.ptr(), stream()) == 0
    assert L.slk_linear_rowstats_f32(x.data_ptr(), K - 1, W.data_ptr(), None, y.ptr(), N, M, K, N, st.ptr(), stream()) == bad
    assert L.slk_linear_rowstats_f32(x.data_ptr(), K, W.data_ptr(), None, y.ptr(), N - 1, M, K, N, st.ptr(), stream()) == bad
    xw = dev(np.ones((M, 129), np.float32))
    assert L.slk_linear_rowstats_f32(xw.data_ptr(), 129, xw.data_ptr(), None, y.ptr(), N, M, 129, 5, st.ptr(),
                                     stream()) == _lib.SLK_ERR_UNSUPPORTED                                           # K = 129
    assert (y.fetch().host == PATTERN).all() and (st.fetch().host == PATTERN).all()


@pytest.mark.parametrize("w_lead", [0, 1])
def test_f32_every_k_exact_on_integers(w_lead):
    """slk_linear_rowstats_f32: all three register counts (K <= 64, 96, 128), K % 4 of every kind, 16-byte and element weight loads."""
    need_gpu()
    for K in pr.F32_SWEEP_K:
        assert pr.paths_f32(pr.SWEEP_M, K, pr.SWEEP_N, w_lead)["wload"] == ("vec16" if K % 4 == 0 and w_lead == 0 else "elem")
        exact32(pr.SWEEP_M, K, pr.SWEEP_N, pr.ALIGNED, w_lead)
        exact32(pr.SWEEP_M, K, pr.SWEEP_N, pr.ODD_LDY, w_lead, bias=False)


@pytest.mark.parametrize("K", pr.F32_TILE_K)
def test_f32_every_tile_count_and_tail_exact(K):
    need_gpu()
    for N in pr.TILE_SWEEP_N:
        exact32(pr.SWEEP_M, K, N, pr.ALIGNED, 0)


@pytest.mark.parametrize("K,N", pr.F32_ROW_KN)
def test_f32_every_row_edge_exact(K, N):
    need_gpu()
    for M in pr.ROW_SWEEP_M:
        exact32(M, K, N, pr.ALIGNED, 0)
        out = exact32(M, K, N, pr.ODD_LDY, 1, stats=False)
        np.testing.assert_array_equal(bits(out), bits(int_case(M, K, N)[3]))


# ------------------------------------------------------------------------------------------------ b. ghost columns
@pytest.mark.parametrize("kernel", ["f16x3", "f32"])
@pytest.mark.parametrize("N", pr.GHOST_N)
def test_ghost_columns_are_neither_counted_nor_stored(kernel, N):
    """Column N - 1, the only column of a partial last tile, holds every row's maximum by a wide margin (every other column sits
    30000 lower).  The tile's 63 ghost columns re-read weight row N - 1; the kernel gives them bias and inverse scale 0, i.e. logit
    0.  A ghost that is counted therefore shows twice: where the row's maximum is negative it becomes the maximum, and everywhere
    it adds exp(-maximum) to a sum that is 1."""
    need_gpu()
    M, K = pr.SWEEP_M, 96
    rs = np.random.RandomState(N)
    x, W = small_ints(rs, M, K), small_ints(rs, N, K)
    b = np.full(N, -30000.0, np.float32)
    b[N - 1] = 0.0
    want = (x.astype(np.int64) @ W.astype(np.int64).T + b.astype(np.int64)).astype(np.float32)
    assert (want.argmax(axis=1) == N - 1).all() and (want[:, N - 1] < -50).sum() > M // 8 and (want[:, N - 1] > 50).sum() > M // 8
    for lay in (pr.ALIGNED, pr.ODD_LDY):
        what = "%s N=%d %s" % (kernel, N, lay)
        out, st = run16(x, Weights(W, b), lay, "stats", what) if kernel == "f16x3" else run32(x, W, b, lay, True, 0, what)
        np.testing.assert_array_equal(bits(out), bits(want), err_msg=what)      # (nothing at column N: checked with the gaps)
        np.testing.assert_array_equal(st[:, 0], want[:, N - 1], err_msg=what)
        np.testing.assert_allclose(1.0 / st[:, 1].astype(np.float64), 1.0, rtol=3e-6, err_msg=what)


# ------------------------------------------------------------------------------------------------ c. float32-grade accuracy
def accuracy_bounds(x, W, b):
    ref, scale = pr.product64(x, W, b), pr.abs_product64(x, W, b)
    model, S = pr.product_split64(x, W, b)
    KP = pr.round_up(x.shape[1], 16)
    # 3 KP float32 additions at one ulp each, in any order and rounding mode, and the final fused multiply-add's share of the bias
    own = 3 * KP * 2.0 ** -23 * S + 2.0 ** -23 * (0.0 if b is None else np.abs(np.asarray(b, np.float64))[None, :])
    return ref, 6e-7 * scale + 1e-6, model, own


@pytest.mark.parametrize("lay", [pr.ALIGNED, pr.ODD_LDY], ids=repr)
def test_f16x3_real_valued_accuracy_per_slab_count(lay):
    """Where lo carries information: against the plain float64 product with the project's bound, 6e-7 sum|x||w| + 1e-6, and against
    the kernel's own three terms in float64 with the worst case of their float32 accumulation, 3 KP 2^-23 S + 2^-23 |b|.
    Largest ratio to the second bound seen per KS on an MI355X: design/fp16_split.md."""
    need_gpu()
    M, N = pr.SWEEP_M, pr.SWEEP_N
    for K in pr.ACCURACY_K:
        x, W, b = real_case(M, K, N)
        out, st = run16(x, Weights(W, b), lay, "stats", "accuracy K=%d %s" % (K, lay))
        assert np.isfinite(out).all()
        ref, bound, model, own = accuracy_bounds(x, W, b)
        e_ref, e_own = np.abs(out.astype(np.float64) - ref), np.abs(out.astype(np.float64) - model)
        print("accuracy %s KS=%d K=%d: ratio to the product bound %.4f, to the accumulation bound %.5f"
              % (lay, (K + 15) // 16, K, (e_ref / bound).max(), (e_own / own).max()))
        assert (e_ref <= bound).all(), (K, float((e_ref / bound).max()))
        assert (e_own <= own).all(), (K, float((e_own / own).max()))
        check_stats(st, out, "accuracy K=%d" % K)


# ------------------------------------------------------------------------------------------------ d. the split kernel
def special_rows(rs, K):
    def with_max(mx, scale):
        r = (rs.uniform(-0.9, 0.9, size=K) * scale).astype(np.float32)
        r[rs.randint(0, K)] = mx
        return r
    p100, p101 = np.float32(2.0 ** -100), np.float32(2.0 ** 101)
    den = rs.randint(1, 2 ** 23, size=K).astype(np.uint32) | (rs.randint(0, 2, size=K).astype(np.uint32) << np.uint32(31))
    return [np.zeros(K, np.float32),                                               # all zero
            den.view(np.float32),                                  # all denormal
            with_max(np.float32(-8.0), 8.0),                       # maximum exactly a power of two
            with_max(p100, p100),                                  # maximum 2^-100: the lower clamp's first in-range value
            with_max(np.nextafter(p100, np.float32(0)), p100),     # ... and just below it
            with_max(-np.nextafter(p101, np.float32(0)), 2.0 ** 100),   # just under 2^101
            with_max(np.float32(1.0), 2.0 ** -13)]                 # hi halves that are fp16 subnormals next to a maximum of 1


@pytest.mark.parametrize("rows", pr.SPLIT_ROWS)
def test_split_kernel_bit_for_bit(rows):
    """slk_split_f16x2_f32 against the numpy model: hi, lo, inverse scales and the zero K padding, bit for bit; 8193 rows is past
    the 2048-block grid's first pass."""
    torch = need_gpu()
    from sloika_amd import _lib
    for K in pr.SPLIT_K:
        rs = np.random.RandomState(rows * 1000 + K)
        sp = special_rows(rs, K)
        base = (rs.normal(size=(rows, K)) * 2.0 ** rs.randint(-60, 60, size=(rows, 1))).astype(np.float32)
        for first in range(0, len(sp), rows):
            w = base.copy()
            take = sp[first:first + rows]
            at = rs.choice(rows, size=len(take), replace=False)    # anywhere: also in the grid's second pass
            w[at] = take
            KP = pr.round_up(K, 16)
            hi, lo = (dev(np.full((rows, KP), 0x7e01, np.uint16).view(np.float16)) for _ in range(2))
            inv = Out(rows, 1, 1)
            wd = dev(w)
            assert _lib.lib().slk_split_f16x2_f32(wd.data_ptr(), rows, K, hi.data_ptr(), lo.data_ptr(), inv.ptr(), stream()) == 0
            whi, wlo, winv = pr.split_f16x2(w)
            what = "rows=%d K=%d specials from %d" % (rows, K, first)
            inv.fetch().assert_untouched_outside(None, what)
            np.testing.assert_array_equal(bits(inv.values().reshape(rows)), bits(winv), err_msg=what)
            ghi, glo = hi.cpu().numpy().view(np.uint16), lo.cpu().numpy().view(np.uint16)
            assert not ghi[:, K:].any() and not glo[:, K:].any(), what + ": K padding"
            np.testing.assert_array_equal(ghi, whi.view(np.uint16), err_msg=what + ": hi")
            np.testing.assert_array_equal(glo, wlo.view(np.uint16), err_msg=what + ": lo")


# ------------------------------------------------------------------------------------------------ e. range ends and containment
def _normalised(a):
    """rows scaled by powers of two so that every row maximum is in [1, 2)"""
    e = np.floor(np.log2(np.abs(a).max(axis=1, keepdims=True)))
    return (a * 2.0 ** -e).astype(np.float32)


def test_f16x3_both_ends_of_the_range():
    """Row maxima in [2^-100, 2^101) are scaled into [1, 2) exactly, so the result is float32-grade wherever the products are
    float32 numbers: rows of x and of W at 2^-100, at 1 and just under 2^101, every pairing whose products neither overflow nor
    leave the normal range.  The project's bound, and the same bound without its absolute term (scaling by powers of two changes no
    significand, so the relative error is that of the unscaled product)."""
    need_gpu()
    M, K, N = 257, 96, 193
    x, W, _ = real_case(M, K, N, seed=1)
    x, W = _normalised(x), _normalised(W)
    ends = np.array([-100.0, 0.0, 100.0])
    ex, ew = ends[np.arange(M) % 3], ends[(np.arange(N) // 3) % 3]
    x, W = (x * 2.0 ** ex[:, None]).astype(np.float32), (W * 2.0 ** ew[:, None]).astype(np.float32)
    x[0] *= np.float32(0.5)
    x[0, np.abs(x[0]).argmax()] = 2.0 ** -100                                               # maximum exactly 2^-100
    x[2, np.abs(x[2]).argmax()] = np.nextafter(np.float32(2.0 ** 101), np.float32(0))       # the last float below 2^101
    assert np.isfinite(x).all() and np.abs(x[0]).max() == 2.0 ** -100 and np.nextafter(np.abs(x[2]).max(), np.float32(np.inf)) == 2.0 ** 101
    keep = np.abs(ex[:, None] + ew[None, :]) <= 100                                         # products in float32's normal range
    assert keep.sum() > 0.7 * M * N
    for lay in (pr.ALIGNED, pr.ODD_LDY):
        out, _ = run16(x, Weights(W, None), lay, "linear", "range ends %s" % lay)
        ref, scale = pr.product64(x, W), pr.abs_product64(x, W)
        err = np.abs(out.astype(np.float64) - ref)
        assert np.isfinite(out[keep]).all()
        assert (err <= 6e-7 * scale + 1e-6)[keep].all()
        assert (err <= 6e-7 * scale)[keep].all(), float((err / scale)[keep].max())


FP16_OVERFLOW = 65520.0 * 2.0 ** 100        # a row maximum from here on scales (by 2^-100, the clamp) to fp16 infinity


@pytest.mark.parametrize("bad", [2.0 ** 101, 2.0 ** 110, 65519.0 * 2.0 ** 100, FP16_OVERFLOW, 2.0 ** 120, 3.0e38, np.inf, np.nan])
@pytest.mark.parametrize("where", ["x row", "W row"])
def test_f16x3_out_of_range_rows_are_contained(where, bad):
    """One entry of one x row, or of one W row, at or above 2^101, infinite or NaN.
    * Its own row (column) never holds a finite wrong number: from 65520 * 2^100 on the scaled entry is fp16 infinity and every
      value of the row (column) is non-finite; below that -- gh_pow2_scale's clamp scales by 2^-100, the scaled maximum lies in
      [2, 65520) and still splits into two finite halves -- the values are finite and float32-grade.
    * Every other row and column keeps the bits it has with a harmless entry in that place; for an x row, the statistics too
      (a W row is a softmax column of every row: the statistics of all rows take part in whatever it holds)."""
    need_gpu()
    M, K, N = 257, 96, 193
    x, W, b = real_case(M, K, N, seed=2)
    r, k = (130, 17) if where == "x row" else (191, 40)
    tgt = x if where == "x row" else W
    base_out, base_st = run16(x, Weights(W, b), pr.ALIGNED, "stats", "baseline")
    tgt[r, k] = bad
    out, st = run16(x, Weights(W, b), pr.ALIGNED, "stats", "%s holds %r" % (where, bad))
    own = out[r, :] if where == "x row" else out[:, r]
    others = np.ones((M, N), bool)
    if where == "x row":
        others[r, :] = False
    else:
        others[:, r] = False
    np.testing.assert_array_equal(bits(out)[others], bits(base_out)[others])
    if where == "x row":
        keep = np.arange(M) != r
        np.testing.assert_array_equal(bits(st)[keep], bits(base_st)[keep])
    if not np.isfinite(bad) or bad >= FP16_OVERFLOW:
        assert not np.isfinite(own).any()
    else:
        # The project's bound, 6e-7 sum|x||w| + 1e-6, is that of rows without an outlier.  Next to one, the other entries' lo halves
        # are fp16 subnormals or zero: hi + lo then holds an entry to 2^-25 of its row's (scaled) maximum, not to 2^-22 of itself
        # (tests/test_projection_ref.py::test_split_reproduces_its_operand), which adds 2^-25 (max|x_r| sum_k |w_nk| + max|w_n|
        # sum_k |x_rk|) -- the term that test_f16x3_operands_of_any_magnitude carries as 1e-6 max|x| max|w| sqrt(K).
        ax, aw = np.abs(x.astype(np.float64)), np.abs(W.astype(np.float64))
        floor = 2.0 ** -25 * (ax.max(axis=1)[:, None] * aw.sum(axis=1)[None, :] + ax.sum(axis=1)[:, None] * aw.max(axis=1)[None, :])
        ref, bound = pr.product64(x, W, b), 6e-7 * pr.abs_product64(x, W, b) + 1e-6 + floor
        ref, bound = (ref[r, :], bound[r, :]) if where == "x row" else (ref[:, r], bound[:, r])
        assert np.isfinite(own).all()
        err = np.abs(own.astype(np.float64) - ref)
        assert (err <= bound).all(), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ f. same bits on repeat
@pytest.mark.parametrize("lay", pr.LAYOUTS, ids=repr)
def test_f16x3_repeats_bit_for_bit(lay):
    """Operand/destination overlap screen (mma()'s empty asm; test_fused_decode_repeats_bit_for_bit is the decoder's): every shape
    of the KS sweep twice into fresh canaried buffers, equal bits in logits and statistics.  One extra launch per shape."""
    need_gpu()
    for K in pr.KS_SWEEP_K:
        x, W, b = real_case(pr.SWEEP_M, K, pr.SWEEP_N, seed=3)
        wt = Weights(W, b)
        a, sa = run16(x, wt, lay, "stats", "first run K=%d" % K)
        c, sc = run16(x, wt, lay, "stats", "second run K=%d" % K)
        assert np.isfinite(a).all(), K
        np.testing.assert_array_equal(bits(a), bits(c), err_msg="K=%d" % K)
        np.testing.assert_array_equal(bits(sa), bits(sc), err_msg="K=%d" % K)
