"""The projection reference model (tests/projection_ref.py) on its own, and the path cover of the shape lists that
tests/test_gpu_projection_edges.py runs: a shape list that stops reaching a kernel path fails here, without a GPU."""
import numpy as np
import pytest

from tests import projection_ref as pr


def _rows(rs, rows, K):
    """Rows of very different magnitudes, an outlier, a zero row."""
    w = rs.normal(size=(rows, K)).astype(np.float32)
    w *= (2.0 ** rs.randint(-90, 90, size=(rows, 1))).astype(np.float32)
    w[0] = 0.0
    if K > 1:
        w[1 % rows, 0] *= 1000.0
    return w


@pytest.mark.parametrize("K", [1, 15, 16, 17, 96, 192])
def test_split_reproduces_its_operand(K):
    """hi + lo is v to 2^-22 |v| where lo is a normal fp16 number and to 2^-25 of the row maximum where it is not."""
    rs = np.random.RandomState(K)
    w = _rows(rs, 64, K)
    hi, lo, inv = pr.split_f16x2(w)
    KP = pr.round_up(K, 16)
    assert hi.shape == lo.shape == (64, KP) and hi.dtype == lo.dtype == np.float16 and inv.dtype == np.float32
    assert not hi[:, K:].any() and not lo[:, K:].any()
    amax = np.abs(w).max(axis=1)
    scaled_max = np.abs(hi.astype(np.float64)).max(axis=1)
    assert ((scaled_max >= 1.0) & (scaled_max <= 2.0))[amax > 0].all() and (scaled_max[amax == 0] == 0).all()
    back = (hi[:, :K].astype(np.float64) + lo[:, :K].astype(np.float64)) * inv[:, None].astype(np.float64)
    err = np.abs(back - w.astype(np.float64))
    normal = np.abs(lo[:, :K].astype(np.float64)) >= 2.0 ** -14
    assert (err[normal] <= 2.0 ** -22 * np.abs(w.astype(np.float64))[normal]).all()
    # lo subnormal or zero: half a subnormal step, 2^-25 in scaled units, where the row maximum is at least 1
    assert (err <= 2.0 ** -25 * amax[:, None].astype(np.float64))[~normal].all()


def test_split_scale_is_the_clamped_exponent():
    sc, inv = pr.pow2_scale(np.array([0.0, 1e-45, 2.0 ** -101, 2.0 ** -100, 1.0, 1.999, 2.0, 2.0 ** 100 * 1.5, 2.0 ** 101, 3e38, np.inf],
                                     np.float32))
    want = np.array([-100, -100, -100, -100, 0, 0, 1, 100, 100, 100, 100])
    np.testing.assert_array_equal(inv, (2.0 ** want).astype(np.float32))
    np.testing.assert_array_equal(sc, (2.0 ** -want).astype(np.float32))
    # ties round to even, subnormal lo halves, NaN stays out of the maximum
    w = np.array([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -23, np.nan]], np.float32)
    hi, lo, inv = pr.split_f16x2(w)
    assert inv[0] == 1.0
    np.testing.assert_array_equal(hi[0, :3].astype(np.float32), [1.0, 1.0 + 2.0 ** -9, 1.0])
    np.testing.assert_array_equal(lo[0, :3].astype(np.float32), [2.0 ** -11, -(2.0 ** -11), 2.0 ** -23])
    assert np.isnan(hi[0, 3]) and np.isnan(lo[0, 3])


@pytest.mark.parametrize("M,K,N", [(33, 1, 5), (40, 17, 70), (64, 96, 129), (50, 192, 65)])
def test_model_against_product(M, K, N):
    """The three kept terms against the plain float64 product: K * 2^-22 * sum |x||w| (the dropped lo.lo term and the halves'
    own rounding are below 2^-22 per product)."""
    rs = np.random.RandomState(M + K + N)
    x = np.tanh(rs.normal(size=(M, K))).astype(np.float32)
    W = (rs.normal(size=(N, K)) * 1.5).astype(np.float32)
    W[0] *= 4.0
    b = rs.normal(size=N).astype(np.float32)
    t, S = pr.product_split64(x, W, b)
    ref, scale = pr.product64(x, W, b), pr.abs_product64(x, W, b)
    assert (np.abs(t - ref) <= K * 2.0 ** -22 * scale).all()
    assert (S <= scale * (1 + 2.0 ** -9)).all() and (S >= 0.99 * pr.abs_product64(x, W)).all()
    m, s = pr.row_stats64(ref.astype(np.float32))
    assert (m == ref.astype(np.float32).max(axis=1)).all() and (s >= 1.0).all() and (s <= N).all()


# ------------------------------------------------------------------------------------------------ path cover
def _all(plans):
    got = set()
    for p in plans:
        got |= pr.combos(p)
    return got


def test_paths_restates_the_dispatch():
    """Hand-checked plans."""
    p = pr.paths(257, 96, 193, 100, 196, stats=True)
    assert (p["ks"], p["ring"], p["xload"], p["xmask"], p["ntiles"], p["nfull"]) == (6, 3, "vec16", False, 4, 3)
    assert [w["fast"] for w in p["wgs"]] == [True, True, False] and [w["rows"] for w in p["wgs"]] == [128, 128, 1]
    assert p["wgs"][0]["tiles"] == [("fast", "patch"), ("fast", "patch"), ("guarded", "guard4"), ("guarded", "dword")]
    assert p["wgs"][0]["pairs"] == 1 and p["wgs"][0]["handover"] == "single"
    assert p["wgs"][2]["tiles"] == [("guarded", "guard4")] * 3 + [("guarded", "dword")] and p["wgs"][2]["handover"] == "single"
    p = pr.paths(128, 176, 132, 176, 132, act="tanh")
    assert (p["ks"], p["ring"], p["xload"]) == (11, 2, "vec16")
    assert p["wgs"][0]["tiles"] == [("fast", "acc4"), ("fast", "acc4"), ("guarded", "tail4")] and p["wgs"][0]["handover"] == "none"
    p = pr.paths(128, 24, 64, 24, 64)
    assert p["xmask"] and p["wgs"][0]["fast"] and p["wgs"][0]["tiles"] == [("guarded", "guard4")] and p["wgs"][0]["pairs"] == 0
    assert pr.paths(128, 24, 64, 24, 65)["wgs"][0]["tiles"] == [("guarded", "dword")]
    assert pr.paths(128, 24, 64, 24, 64, y_lead=1)["wgs"][0]["tiles"] == [("guarded", "dword")]
    assert pr.paths(128, 24, 64, 24, 64, x_lead=1)["xload"] == "elem" and pr.paths(128, 24, 64, 25, 64)["xload"] == "elem"
    assert pr.paths(1, 20, 64, 20, 64)["xload"] == "elem"
    assert pr.paths_f32(257, 64, 5)["areg"] == 32 and pr.paths_f32(257, 65, 5)["areg"] == 48 and pr.paths_f32(1, 97, 5)["areg"] == 64
    assert pr.paths_f32(1, 129, 5)["areg"] is None and pr.paths_f32(1, 64, 5, w_lead=1)["wload"] == "elem"


def test_ks_sweep_reaches_every_slab_load_and_store():
    M, N = pr.SWEEP_M, pr.SWEEP_N
    plans = {(lay.name, K): lay.paths(M, K, N, stats=True) for lay in pr.LAYOUTS for K in pr.KS_SWEEP_K}
    got = _all(plans.values())
    for ks in range(1, 13):
        ring = 3 if ks <= 9 else 2
        fast_store = "patch" if ks <= 8 else "acc4"
        mine_got = {c for c in got if c[0] == ks}
        assert {c[1] for c in mine_got} == {ring} and {c[4] for c in mine_got} == {"vec16", "elem"}, ks
        # the x load and the store path are independent code: each store under some x load (K = 64 and 96 are their slab
        # counts' only members, so an element load never meets a float4 store there)
        assert {(c[2], c[3]) for c in mine_got} == {("fast", fast_store), ("guarded", "guard4"), ("guarded", "dword")}, ks
        mine = [K % 16 for K in pr.KS_SWEEP_K if pr.round_up(K, 16) == 16 * ks]
        assert 0 in mine, ks                                       # a whole last slab ...
        assert any(mine) or ks in (4, 6), ks                       # ... and a masked one (the list holds no K in 49..63, 81..95)
    # K % 16: full slab, one element, the lower lane half alone, all but one element
    assert {K % 16 for K in pr.KS_SWEEP_K} >= {0, 1, 8, 15}
    # the 16-byte x load with the upper lane half of the last slab masked off
    assert {plans[("aligned", K)]["ks"] for K in pr.KS_SWEEP_K if K % 16 == 8 and plans[("aligned", K)]["xload"] == "vec16"} == {1, 2, 3, 5, 9}
    for K in pr.KS_SWEEP_K:
        # an odd stride or a pointer one float off: guarded epilogue and dword stores only
        for name in ("odd_ldy", "off_one"):
            assert {s for wg in plans[(name, K)]["wgs"] for s in wg["tiles"]} == {("guarded", "dword")}, (name, K)
        assert plans[("off_one", K)]["xload"] == "elem"
        assert plans[("odd_ldy", K)]["xload"] == plans[("aligned", K)]["xload"] == ("vec16" if K % 8 == 0 else "elem")
        # full and ragged workgroups in one launch
        assert [w["fast"] for w in plans[("aligned", K)]["wgs"]] == [True, True, False]


def test_tile_sweep_reaches_every_tile_count_and_tail():
    for K in pr.TILE_SWEEP_K:
        plans = [pr.ALIGNED.paths(pr.SWEEP_M, K, N, stats=True) for N in pr.TILE_SWEEP_N]
        ring = 3 if K <= 144 else 2
        assert {p["ring"] for p in plans} == {ring}
        assert {p["nfull"] for p in plans} == set(range(0, 7)) and {p["ntiles"] for p in plans} == set(range(1, 8))
        fast = [p["wgs"][0] for p in plans]
        assert all(w["fast"] for w in fast)
        assert {w["pairs"] for w in fast} == {0, 1, 2, 3}
        # every pass count of the two-tile loop hands over to nothing but the last epilogue, and to one leftover tile
        assert {(w["pairs"], w["handover"]) for w in fast} == {(p, h) for p in (0, 1, 2) for h in ("none", "single")} | {(3, "none")}
        stores = {s for w in fast for (_, s) in w["tiles"]}
        assert stores == {"patch" if ring == 3 else "acc4", "guard4", "tail4", "dword"}
        # a full tile left over in a fast workgroup leaves through the guarded float4 store, next to fast tiles
        assert any(("fast", "patch" if ring == 3 else "acc4") in w["tiles"] and ("guarded", "guard4") in w["tiles"] for w in fast)
        # the partial tile as the N % 4 == 0 store and as dwords, alone (one tile, no second prefetch) and behind full tiles
        assert any(p["ntiles"] == 1 and p["wgs"][0]["tiles"] == [("guarded", "tail4")] for p in plans)
        assert any(p["ntiles"] == 1 and p["wgs"][0]["tiles"] == [("guarded", "dword")] for p in plans)
        assert any(p["ntiles"] == 1 and p["wgs"][0]["tiles"] == [("guarded", "guard4")] for p in plans)
        ragged = [p["wgs"][-1] for p in plans]
        assert not any(w["fast"] for w in ragged) and {s for w in ragged for (_, s) in w["tiles"]} == {"guard4", "tail4", "dword"}
        assert {w["handover"] for w in ragged} == {"none", "single", "double"}


def test_row_sweep_reaches_every_row_edge():
    for (K, N) in pr.ROW_SWEEP_KN:
        plans = {M: pr.ALIGNED.paths(M, K, N, stats=True) for M in pr.ROW_SWEEP_M}
        assert {p["wgs"][-1]["rows"] for p in plans.values()} == {1, 31, 32, 33, 127, 128}
        assert [w["fast"] for w in plans[128]["wgs"]] == [True] and [w["fast"] for w in plans[127]["wgs"]] == [False]
        assert [w["fast"] for w in plans[129]["wgs"]] == [True, False] and [w["fast"] for w in plans[256]["wgs"]] == [True, True]
        assert [w["fast"] for w in plans[257]["wgs"]] == [True, True, False] and [w["fast"] for w in plans[255]["wgs"]] == [True, False]
    assert {pr.paths_f32(M, 96, 129)["rows_last"] for M in pr.ROW_SWEEP_M} == {1, 31, 32, 33, 127, 128}


def test_activation_shapes_reach_every_store_in_every_instantiation():
    for mode in pr.MODES:
        got = _all(pr.mode_paths(pr.ALIGNED, M, K, N, mode) for (M, K, N) in pr.ACT_SHAPES)
        want = {(6, 3, "fast", "patch", "vec16", mode), (6, 3, "guarded", "guard4", "vec16", mode), (6, 3, "guarded", "dword", "vec16", mode),
                (11, 2, "fast", "acc4", "vec16", mode), (11, 2, "guarded", "tail4", "vec16", mode),
                (2, 3, "guarded", "guard4", "vec16", mode)}
        assert got >= want, (mode, want - got)
        assert {s for c in got for s in (c[3],)} == set(pr.STORES)


def test_remaining_lists_reach_what_they_claim():
    # ghost columns: a partial last tile behind 1, 2 and 3 full ones, dword tail, in a fast and in a ragged workgroup
    for N in pr.GHOST_N:
        p = pr.ALIGNED.paths(pr.SWEEP_M, 96, N, stats=True)
        assert N % 64 == 1 and p["nfull"] == N // 64 and p["wgs"][0]["tiles"][-1] == ("guarded", "dword") and not p["wgs"][-1]["fast"]
    # accuracy: one 16-byte-loadable K per slab count
    assert [(K + 15) // 16 for K in pr.ACCURACY_K] == list(range(1, 13)) and all(K % 8 == 0 for K in pr.ACCURACY_K)
    assert any(K % 16 == 8 for K in pr.ACCURACY_K)
    # the float32 twin: all three register counts, both weight loads
    got = {(pr.paths_f32(pr.SWEEP_M, K, pr.SWEEP_N, lead)["areg"], pr.paths_f32(pr.SWEEP_M, K, pr.SWEEP_N, lead)["wload"])
           for K in pr.F32_SWEEP_K for lead in (0, 1)}
    assert got == {(a, w) for a in (32, 48, 64) for w in ("vec16", "elem")}
    assert {pr.paths_f32(1, K, 1)["areg"] for K in pr.F32_TILE_K} == {48, 64} and {pr.paths_f32(1, K, 1)["areg"] for K, _ in pr.F32_ROW_KN} == {48, 64}
    assert pr.paths_f32(1, pr.K_MAX_F32 + 1, 1)["areg"] is None
    assert {pr.paths_f32(pr.SWEEP_M, 65, N)["ntiles"] for N in pr.TILE_SWEEP_N} == set(range(1, 8))
    # the split kernel: more rows than its grid covers in one pass (4 rows per block, 2048 blocks), K around the 64-lane stride
    assert max(pr.SPLIT_ROWS) > 4 * 2048 and {K % 16 for K in pr.SPLIT_K} >= {0, 1, 15} and max(pr.SPLIT_K) == pr.K_MAX
