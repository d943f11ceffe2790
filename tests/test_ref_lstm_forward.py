"""tests/ref_lstm_forward.py on the CPU: the float64 recursion against oracle_np.lstm, the C oracle and the reference's own layer outputs
under tests/golden/, so that it is no third opinion of unknown standing; the case tables the GPU tests run, every entry admitted by
its own yardstick and laid around the geometry the kernel sources declare; and the checker, which must be able to fail -- shown
with single elements moved by 1e-5 (inside the 2e-5 the existing Lstm tests allow) and with three recursions made wrong on purpose."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import ref_layers
from tests import ref_lstm_forward as rl

F32, F64 = np.float32, np.float64
GRADES = [(F64, None), (F32, None), (F32, 22)]


def _small(seed, T=11, B=4, I=5, n=7):
    rs = np.random.RandomState(seed)
    iW, sW, b, p = (rs.normal(size=s) * 0.8 for s in ((4 * n, I), (4 * n, n), (4 * n,), (3, n)))
    return rs.normal(size=(T, B, I)), iW, sW, b, p


# --------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("reverse", [False, True])
def test_float64_recursion_equals_oracle_np(reverse):
    x, iW, sW, b, p = _small(3 + reverse)
    for bias, peep in ((b, p), (None, p), (b, None), (None, None)):
        h = rl.lstm_forward(x, iW, sW, bias, peep, reverse)
        assert h.dtype == F64 and h.shape == (11, 4, 7)
        assert np.abs(h - oracle_np.lstm(x, iW, sW, bias, peep, reverse=reverse)).max() <= 1e-12
    act, gate = rl.OTHER_PAIR
    h = rl.lstm_forward(x, iW, sW, b, p, reverse, act=act, gate=gate)
    assert np.abs(h - oracle_np.lstm(x, iW, sW, b, p, act=act, gate=gate, reverse=reverse)).max() <= 1e-12
    assert np.abs(h - rl.lstm_forward(x, iW, sW, b, p, reverse)).max() > 1e-3          # ... and the pair is another function


@pytest.mark.parametrize("reverse", [False, True])
def test_float64_recursion_equals_c_oracle(oracle, reverse):
    """Within the C oracle's own float32 error: the 2e-5 tests/test_oracle_reference_layers.py holds it to."""
    c = rl.layer_case(36, 48, "moderate", 13, rl.EDGE_B, reverse)
    ref = oracle.lstm(c["x"], c["iW"], c["sW"], c["b"], c["p"], reverse=reverse)
    assert np.abs(c["h"] - ref).max() <= 2e-5


def _lstm_leaf(tree):
    rev = tree["type"] == "reverse"
    leaf = tree["sublayer"] if rev else tree
    return (leaf, rev) if leaf["type"] == "LSTM" else (None, rev)


LSTM_FIXTURES = sorted(k for k, v in ref_layers.meta()["layers"].items() if _lstm_leaf(v["tree"])[0] is not None)


@pytest.mark.parametrize("name", LSTM_FIXTURES)
def test_float64_recursion_equals_the_reference_layers_own_output(name):
    """tests/golden/layers.npz: what sloika/layers.py's Lstm itself produced, at tests/test_oracle_reference_layers.py's 1e-10."""
    lc = ref_layers.lc
    case = ref_layers.meta()["layers"][name]
    ref_layers.check_inputs(case)
    leaf, reverse = _lstm_leaf(lc.materialise(case["tree"], F64))
    assert leaf["activation"] == "tanh" and leaf["gate"] == "sigmoid"
    x = lc.expand(case["x"]).astype(F64)
    h = rl.lstm_forward(x, leaf["iW"], leaf["sW"], leaf.get("b"), leaf.get("p"), reverse)
    np.testing.assert_allclose(h, ref_layers.arrays()["layer/" + name], rtol=0, atol=1e-10)


def test_the_fixtures_hold_what_is_claimed():
    assert len(LSTM_FIXTURES) >= 10 and any(n.endswith("_rev") for n in LSTM_FIXTURES)
    forms = {(ref_layers.meta()["layers"][n]["tree"].get("b") is not None, ref_layers.meta()["layers"][n]["tree"].get("p") is not None)
             for n in LSTM_FIXTURES if not n.endswith("_rev")}
    assert {(True, True), (True, False), (False, False)} <= forms


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("grade", GRADES)
def test_each_ragged_chunk_equals_the_call_on_the_chunk_alone(reverse, grade):
    x, iW, sW, b, p = _small(17)
    lens = np.array([11, 1, 6, 10])
    h = rl.lstm_forward(x, iW, sW, b, p, reverse, lens, *grade)
    assert h.dtype == grade[0]
    for bb, tb in enumerate(lens):
        h1 = rl.lstm_forward(x[:tb, bb:bb + 1], iW, sW, b, p, reverse, None, *grade)
        # (to rounding: a product of four rows and of one are different BLAS calls and sum in different orders)
        assert np.abs(h[:tb, bb:bb + 1] - h1).max() <= (1e-12 if grade[0] == F64 else 5e-6)
        assert np.isnan(h[tb:, bb]).all()                                         # MARKER
    full = rl.lstm_forward(x, iW, sW, b, p, reverse, np.full(4, 11), *grade)
    assert np.array_equal(full, rl.lstm_forward(x, iW, sW, b, p, reverse, None, *grade))


@pytest.mark.parametrize("reverse", [False, True])
def test_projection_handed_over_is_the_same_recursion(reverse):
    x, iW, sW, b, p = _small(23)
    lens = np.array([11, 1, 6, 10])
    for ln in (None, lens):
        h = rl.lstm_forward(x, iW, sW, b, p, reverse, ln)
        hv = rl.lstm_forward(None, None, sW, None, p, reverse, ln, vW=x @ iW.T + b)
        assert np.array_equal(np.isnan(h), np.isnan(hv)) and np.abs(np.nan_to_num(h - hv)).max() <= 1e-14


def test_yardsticks_are_float32_and_coarser_than_float64():
    c = rl.layer_case(64, 64, "moderate", 9, rl.EDGE_B, False)
    y32 = rl.lstm_forward(c["x"], c["iW"], c["sW"], c["b"], c["p"], False, None, F32)
    assert y32.dtype == F32 and c["hy"].dtype == F32 and c["grade"] == "y22"
    e32, e22 = np.abs(y32 - c["h"]).max(), np.abs(c["hy"] - c["h"]).max()
    assert 2.0 ** -26 < e32 < 2e-6 and 2.0 ** -26 < e22 < 2e-6, (e32, e22)
    assert not np.array_equal(y32, c["hy"])                                       # the operand rounding does something
    s = rl.scan_case(64, 9, rl.EDGE_B, False)
    s32 = rl.scan_case(64, 9, rl.EDGE_B, False, None, True, "y32")
    assert np.array_equal(s["h"], s32["h"]) and not np.array_equal(s["hy"], s32["hy"]) and s32["grade"] == "y32"
    assert s["vW"].dtype == F32 and s["hy"].dtype == F32 and s32["hy"].dtype == F32


# ------------------------------------------------------------------------------------------------------ the tables
def test_generators_are_the_distributions_they_name():
    iW, sW, b, p = rl.weights(12, 64, "moderate")
    assert all(a.dtype == F32 for a in (iW, sW, b, p)) and iW.shape == (256, 12) and sW.shape == (256, 64) and p.shape == (3, 64)
    assert abs(sW.std() * np.sqrt(128) - 2.0) < 0.1 and abs(iW.std() * np.sqrt(76) - 1.0) < 0.05 and abs(p.std() * 8 - 1.0) < 0.2
    tiW, tsW, _, _ = rl.weights(12, 64, "trained")
    assert np.abs(tsW).max() == 6.0 and 50 <= np.isin(tsW, [-6.0, 5.0, 4.5]).sum() <= 60 and abs(tiW.std() * np.sqrt(76) - 2.0) < 0.1
    plain, mixed = rl.layer_case(12, 64, "moderate", 13, rl.EDGE_B, False), rl.layer_case(12, 64, "moderate", 13, rl.EDGE_B, False, None, True)
    changed = np.argwhere((plain["x"] != mixed["x"]).any(axis=2))
    assert changed.tolist() == [[5, 1], [6, 2]]                                   # two rows of the group of steps 4 .. 7
    assert np.allclose(mixed["x"][5, 1], plain["x"][5, 1] * 1e-3) and np.allclose(mixed["x"][6, 2], plain["x"][6, 2] * 1e3)
    assert rl.layer_case(12, 64, "moderate", 9, 17, False, None, False, False, True)["b"] is None
    assert rl.layer_case(12, 64, "moderate", 9, 17, False, None, False, True, False)["p"] is None


def test_mixed_yardstick_is_the_worst_of_its_summation_orders():
    orders = rl.summation_orders(60)
    assert len(orders) == 4 and all(sorted(k) == list(range(60)) for k in orders) and orders[0].tolist() == list(range(60))
    assert len({tuple(k) for k in orders}) == 4
    c = rl.layer_case(60, 64, "moderate", 6, rl.EDGE_B, False, None, True)
    given = rl.lstm_forward(c["x"], c["iW"], c["sW"], c["b"], c["p"], False, None, F32, 22)
    assert c["yard"] >= rl.chunk_errors(given, c["h"], None).max()
    # the same arithmetic in another order is the same recursion: within float32 of each other where nothing is ill-conditioned
    plain = rl.layer_case(60, 64, "moderate", 6, rl.EDGE_B, False)
    k = orders[2]
    moved = rl.lstm_forward(np.ascontiguousarray(plain["x"][:, :, k]), np.ascontiguousarray(plain["iW"][:, k]), plain["sW"], plain["b"],
                            plain["p"], False, None, F32, 22)
    assert np.abs(moved - plain["hy"]).max() < 2e-6


def test_time_edges_follow_the_kernels_declared_geometry():
    """The constants as the kernel sources state them, and the lengths they demand of the tables."""
    geo = rl.declared_geometry()
    assert geo == {"KB": 8, "fused_group": 4, "fused_ahead": 2, "scan_unroll": 4, "scan_sets": 4, "scan_ahead": 3}, geo
    assert geo["scan_ahead"] == geo["scan_sets"] - 1 and geo["scan_unroll"] == geo["scan_sets"]
    tables = {"EDGE_T (fused16)": rl.EDGE_T, "EDGE_T (scan16)": rl.EDGE_T, "MFMA_T": rl.MFMA_T}
    for name, (want, constant) in rl.demanded_edges(geo).items():
        missing = sorted(want - set(tables[name]))
        assert not missing, "%s lacks T = %s, which %s demands" % (name, missing, constant)
    assert set(rl.MFMA_T) == rl.demanded_edges(geo)["MFMA_T"][0]
    assert {T % 4 for T in rl.EDGE_T} == {0, 1, 2, 3} and {T % 8 for T in rl.MFMA_T} >= {0, 1, 7}
    # a kernel with other constants gets other tables
    moved = rl.demanded_edges(dict(geo, KB=4, fused_group=2, scan_sets=8))
    assert not moved["MFMA_T"][0] <= set(rl.MFMA_T) and not moved["EDGE_T (scan16)"][0] <= set(rl.EDGE_T)
    assert moved["EDGE_T (fused16)"][0] <= set(rl.EDGE_T)                          # (shorter groups: already inside)


def test_ragged_lengths_cover_what_they_claim():
    for lens, lengths, T in ((rl.ragged_lens(), rl.RAGGED_LENGTHS, rl.RAGGED_T), (rl.mfma_ragged_lens(), rl.MFMA_RAGGED_LENGTHS, rl.MFMA_RAGGED_T)):
        assert len(lens) == rl.RAGGED_B == 17 and max(lens) == T and set(lens) == set(lengths) and lens[-1] == 1
        for slot in range(4):
            seen = {lens[b] for b in range(slot, 16, 4)}
            assert len(seen) == 4 and min(seen) < T                               # every slot of a workgroup sees short chunks
        assert any(len(set(lens[g:g + 4])) == 4 and max(lens[g:g + 4]) == T for g in range(0, 16, 4))     # the full chunk beside short ones
    kb = rl.declared_geometry()["KB"]
    assert {kb - 1, kb, kb + 1, 2 * kb - 1, 2 * kb, 2 * kb + 1, 3 * kb, 3 * kb + 1} <= set(rl.MFMA_RAGGED_LENGTHS)
    assert len(rl.GENERIC_LENS) == max(rl.GENERIC_B) and max(rl.GENERIC_LENS) == max(rl.GENERIC_T) and 1 in rl.GENERIC_LENS
    assert set(rl.BATCH_B) >= {1, 2, 3, 4, 5, 7, 8, 9}                            # 1 .. 3 live chunks in the last workgroup, 0 dead


def test_trained_and_mixed_tables_are_subsets_of_what_was_asked():
    for asked, table in ((rl.TRAINED_T_ASKED, rl.EDGE_T_TRAINED), (rl.MIXED_T_ASKED, rl.EDGE_T_MIXED)):
        assert set(table) == set(rl.FUSED_SHAPES)
        for ts in table.values():                                                 # an entry is an asked length or lies in its group of four
            assert ts and all(any((T - 1) // 4 == (a - 1) // 4 and T <= a for a in asked) for T in ts)
    assert all(1 in ts for ts in rl.EDGE_T_TRAINED.values())
    assert 0 < rl.TABLE_MARGIN < 1


@pytest.mark.parametrize("I,n", rl.FUSED_SHAPES)
def test_every_listed_layer_case_is_admitted(I, n):
    """y22 of every case the GPU tests list for the shape, on that case's own inputs, is at most CAP / 8."""
    mine = [a for a in rl.listed_layer_cases() if a[:2] == (I, n)]
    assert len(mine) >= 2 * (len(rl.EDGE_T) + len(rl.TRAINED_T_ASKED) + len(rl.MIXED_T_ASKED) + 5)
    for args in mine:
        c = rl.layer_case(*args)
        own = np.arange(c["T"])[:, None] < (np.full(c["B"], c["T"]) if c["lens"] is None else c["lens"])[None, :]
        assert np.isfinite(c["h"][own]).all() and np.isfinite(c["x"]).all()
        assert c["yard"] <= rl.ADMIT, (args, c["yard"])


@pytest.mark.parametrize("grade", ["y22", "y32"])
def test_every_listed_scan_case_is_admitted(grade):
    mine = [a for a in rl.listed_scan_cases() if (a[6] if len(a) > 6 else "y22") == grade]
    assert len(mine) > 100
    for args in mine:
        c = rl.scan_case(*args)
        assert c["grade"] == grade and np.isfinite(c["vW"]).all()
        assert c["yard"] <= rl.ADMIT, (args, c["yard"])
    for I, n in rl.GEMM_SHAPES:
        assert rl.gemm_case(I, n, rl.BATCH_T, 5, True)["yard"] <= rl.ADMIT


# ----------------------------------------------------------------------------------------------------- the checker
def _ragged(reverse):
    return rl.layer_case(36, 48, "moderate", rl.RAGGED_T, rl.RAGGED_B, reverse, rl.ragged_lens())


def test_checker_accepts_the_reference_and_the_yardstick(capsys):
    for reverse in (False, True):
        c = _ragged(reverse)
        rl.check(c["h"], c, "self")
        rl.check(c["hy"], c, "y22")
        rl.check(c["h"].astype(F32), c, "rounded")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("LSTMFWD ")]
    assert len(lines) == 6 and all(" ratio " in l and " chunk " in l and " bound " in l and " yardstick y22 " in l for l in lines)
    c = rl.layer_case(36, 48, "moderate", rl.BATCH_T, max(rl.BATCH_B), False)
    small = c.take(3)
    assert small["h"].shape[1] == 3 and small["B"] == 3 and c["B"] == 9 and small["x"].shape[1] == 3
    assert small["yard"] == rl.chunk_errors(c["hy"][:, :3], c["h"][:, :3], None).max() <= c["yard"]
    rl.check(small["h"], small, "first three chunks")


def test_checker_rejects_one_element_moved_by_1e_5():
    c = rl.layer_case(36, 48, "moderate", 9, rl.EDGE_B, True)
    got = c["h"].copy()
    got[4, 11, 7] += 1e-5
    with pytest.raises(AssertionError, match="chunk 11"):
        rl.check(got, c, "moved")
    c = _ragged(True)
    got = c["h"].copy()
    got[0, 16, 3] -= 1e-5                                                         # the only step of the last chunk
    with pytest.raises(AssertionError, match="chunk 16"):
        rl.check(got, c, "moved")
    got = c["h"].copy()
    got[1, 16, 3] = 0.5                                                           # ... while behind a chunk's end nothing is compared
    rl.check(got, c, "behind the end")
    got = c["h"].copy()
    assert c["lens"][3] == 4
    got[2, 3, 0] = np.nan
    with pytest.raises(AssertionError, match="chunk 3"):
        rl.check(got, c, "nan")
    with pytest.raises(AssertionError, match="beyond the suite's"):                # the cap holds whatever the yardstick says
        loose = rl.Case(**c)
        loose["yard"] = 1.0
        rl.check(c["h"] + 3e-5, loose, "cap")


@pytest.mark.parametrize("reverse", [False, True])
def test_checker_rejects_a_chunk_one_step_short_or_started_at_the_batch_end(reverse):
    c = _ragged(reverse)
    for victim in (6, 10):                                                        # lengths 9 and 17
        lens = c["lens"].copy()
        lens[victim] -= 1
        h = rl.lstm_forward(c["x"], c["iW"], c["sW"], c["b"], c["p"], reverse, lens)
        with pytest.raises(AssertionError, match="chunk %d" % victim):
            rl.check(h, c, "short")
        with pytest.raises(AssertionError, match="chunk %d" % victim):             # also where the missing row holds something finite
            rl.check(np.nan_to_num(h, nan=0.0), c, "short, zero-filled")
    if reverse:
        for victim in (0, 9, 16):                                                 # lengths 1, 16 and 1
            tb = int(c["lens"][victim])
            h = c["h"].copy()
            h[:tb, victim:victim + 1] = rl.lstm_forward(c["x"][:, victim:victim + 1], c["iW"], c["sW"], c["b"], c["p"], True)[:tb]
            with pytest.raises(AssertionError, match="chunk %d" % victim):
                rl.check(h, c, "started at T - 1")


# ------------------------------------------------------------------------------------------ arithmetic wrong on purpose
def _hi_half(W):
    """Every row scaled into [1, 2) and rounded to ONE fp16: the hi half of the pair, the lo half dropped."""
    W = np.asarray(W, F64)
    _, ex = np.frexp(np.abs(W).max(axis=1, keepdims=True))
    sc = np.ldexp(1.0, 1 - ex)
    return (W * sc).astype(np.float16).astype(F64) / sc


def _sabotaged(c, kind):
    """The float64 recursion of a full-length case with one thing wrong:
    "lo dropped": the recurrent weights at fp16 precision;  "stale state": step 9 (the second of the third group of four) multiplies
    the output of step 7 in place of step 8's;  "old cell": the output gate peeps at the cell state before the update."""
    assert c["lens"] is None and c["T"] >= 12
    x, iW, sW, b, p = (np.asarray(c[k], F64) for k in ("x", "iW", "sW", "b", "p"))
    T, B, n = c["T"], c["B"], c["n"]
    if kind == "lo dropped":
        sW = _hi_half(sW)
    h = np.empty((T, B, n))
    outs, cell = [np.zeros((B, n))], np.zeros((B, n))
    for s in range(T):
        t = T - 1 - s if c["reverse"] else s
        prev = outs[-2] if kind == "stale state" and s == 9 else outs[-1]
        a = (x[t] @ iW.T + b + prev @ sW.T).reshape(B, n, 4)
        cn = cell * rl.sigmoid(a[:, :, 2] + cell * p[1]) + np.tanh(a[:, :, 0]) * rl.sigmoid(a[:, :, 1] + cell * p[0])
        hn = np.tanh(cn) * rl.sigmoid(a[:, :, 3] + (cell if kind == "old cell" else cn) * p[2])
        outs.append(hn)
        cell, h[t] = cn, hn
    return h


@pytest.mark.parametrize("reverse", [False, True])
def test_the_sabotage_loop_is_the_reference_when_nothing_is_wrong(reverse):
    c = rl.layer_case(12, 64, "moderate", 13, rl.EDGE_B, reverse)
    assert np.abs(_sabotaged(c, None) - c["h"]).max() <= 1e-14


@pytest.mark.parametrize("kind", ["lo dropped", "stale state", "old cell"])
@pytest.mark.parametrize("I,n", [(12, 64), (4, 16)])
def test_checker_rejects_wrong_arithmetic(I, n, kind):
    """Each wrong recursion fails `check` in EVERY chunk of listed `moderate` cases (T = 13 and 17, both directions).  Printed beside
    each error: how many chunks the 2e-5 of the existing Lstm tests would pass.  As measured: none.  A dropped lo half costs 1e-4 to
    5e-4 here (6e-5 to 2e-4 at T = 2 and 3), five to twenty-five times the old tolerance and a hundred to four hundred times the
    bound; a stale state 2e-2 to 3e-1; the old cell under the output gate 2e-2 to 6e-2.  What the old tolerance does let through and the
    bound does not is an error of 1e-6 to 2e-5: test_checker_rejects_one_element_moved_by_1e_5."""
    for T in (13, 17):
        for reverse in (False, True):
            c = rl.layer_case(I, n, "moderate", T, rl.EDGE_B, reverse)
            assert (I, n, "moderate", T, rl.EDGE_B, reverse, None, False) in rl.listed_layer_cases()
            h = _sabotaged(c, kind)
            err = rl.chunk_errors(h, c["h"], None)
            bound = rl.BOUND[0] * c["yard"] + rl.BOUND[1]
            print("LSTMFWD-SABOTAGE %s (%d,%d) T=%d rev=%d: worst chunk %.3e, best chunk %.3e, bound %.3e; chunks the old 2e-5 passes: %d of %d"
                  % (kind, I, n, T, reverse, err.max(), err.min(), bound, (err < rl.CAP).sum(), len(err)))
            assert err.min() > bound                                              # EVERY chunk shows it
            with pytest.raises(AssertionError, match="allows"):
                rl.check(h, c, kind)
