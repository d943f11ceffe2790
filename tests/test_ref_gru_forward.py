"""tests/ref_gru_forward.py on the CPU: the float64 recursion against oracle_np.gru and the C oracle (both pinned to the reference's
layers.py elsewhere in the suite), so that it is no third opinion of unknown standing; the case tables the GPU tests run, every entry
admitted by its own yardstick; and the checker, which must be able to fail."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import ref_gru_forward as rg

F32, F64 = np.float32, np.float64


def _small(seed, T=11, B=4, I=5, n=7):
    rs = np.random.RandomState(seed)
    iW, sW, sW2, b = (rs.normal(size=s) * 0.8 for s in ((3 * n, I), (2 * n, n), (n, n), (3 * n,)))
    return rs.normal(size=(T, B, I)), iW, sW, sW2, b


# --------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("reverse", [False, True])
def test_float64_recursion_equals_oracle_np(reverse):
    x, iW, sW, sW2, b = _small(3 + reverse)
    h, zr = rg.gru_forward(x, iW, sW, sW2, b, reverse)
    assert h.dtype == F64 and zr.shape == (11, 4, 14)
    assert np.abs(h - oracle_np.gru(x, iW, sW, sW2, b, reverse=reverse)).max() <= 1e-12
    assert np.abs(rg.gru_forward(x, iW, sW, sW2, None, reverse)[0] - oracle_np.gru(x, iW, sW, sW2, None, reverse=reverse)).max() <= 1e-12
    # the projection handed in (the wide layers' scan) is the same recursion
    vI = x @ iW.T + b
    hv, zrv = rg.gru_forward(None, None, sW, sW2, None, reverse, vI=vI)
    assert np.array_equal(hv, h) and np.array_equal(zrv, zr)


@pytest.mark.parametrize("reverse", [False, True])
def test_float64_recursion_equals_c_oracle(oracle, reverse):
    c = rg.layer_case(48, 32, "moderate", 13, rg.EDGE_B, reverse)
    ref = oracle.gru(c["x"], c["iW"], c["sW"], c["sW2"], c["b"], reverse=reverse)
    assert np.abs(c["h"] - ref).max() <= 2e-5


@pytest.mark.parametrize("reverse", [False, True])
def test_saved_gates_satisfy_the_blend(reverse):
    """h_t = z h_{t-1} + (1 - z) c with the float64 candidate c = tanh(vI_c + (r h_{t-1}) sW2^T), h_{t-1} the previous SCAN step."""
    x, iW, sW, sW2, b = _small(9 + reverse)
    n = sW2.shape[0]
    h, zr = rg.gru_forward(x, iW, sW, sW2, b, reverse)
    hs, zs, xs = (a[::-1] if reverse else a for a in (h, zr, x))
    hprev = np.concatenate([np.zeros((1,) + h.shape[1:]), hs[:-1]], axis=0)
    z, r = zs[..., :n], zs[..., n:]
    assert (z > 0).all() and (z < 1).all() and (r > 0).all() and (r < 1).all()
    c = np.tanh((xs @ iW.T + b)[..., 2 * n:] + (r * hprev) @ sW2.T)
    assert np.abs(hs - (z * hprev + (1 - z) * c)).max() <= 1e-14
    vS = hprev @ sW.T
    assert np.abs(z - rg.sigmoid((xs @ iW.T + b)[..., :n] + vS[..., :n])).max() <= 1e-14
    assert np.abs(r - rg.sigmoid((xs @ iW.T + b)[..., n:2 * n] + vS[..., n:])).max() <= 1e-14


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("grade", [(F64, None), (F32, None), (F32, 22)])
def test_each_ragged_chunk_equals_the_call_on_the_chunk_alone(reverse, grade):
    x, iW, sW, sW2, b = _small(17)
    lens = np.array([11, 1, 6, 10])
    h, zr = rg.gru_forward(x, iW, sW, sW2, b, reverse, lens, *grade)
    assert h.dtype == grade[0]
    for bb, tb in enumerate(lens):
        h1, zr1 = rg.gru_forward(x[:tb, bb:bb + 1], iW, sW, sW2, b, reverse, None, *grade)
        # (to rounding: a product of four rows and of one are different BLAS calls and sum in different orders)
        tol = 1e-12 if grade[0] == F64 else 5e-6
        assert np.abs(h[:tb, bb:bb + 1] - h1).max() <= tol and np.abs(zr[:tb, bb:bb + 1] - zr1).max() <= tol
        assert np.isnan(h[tb:, bb]).all() and np.isnan(zr[tb:, bb]).all()         # MARKER
    full = rg.gru_forward(x, iW, sW, sW2, b, reverse, np.full(4, 11), *grade)
    none = rg.gru_forward(x, iW, sW, sW2, b, reverse, None, *grade)
    assert np.array_equal(full[0], none[0]) and np.array_equal(full[1], none[1])


def test_yardsticks_are_float32_and_coarser_than_float64():
    c = rg.layer_case(64, 64, "moderate", 9, rg.EDGE_B, False)
    y32 = rg.gru_forward(c["x"], c["iW"], c["sW"], c["sW2"], c["b"], False, None, F32)[0]
    assert y32.dtype == F32 and c["h22"].dtype == F32 and c["zr22"].dtype == F32
    e32, e22 = np.abs(y32 - c["h"]).max(), np.abs(c["h22"] - c["h"]).max()
    assert 2.0 ** -26 < e32 < 2e-6 and 2.0 ** -26 < e22 < 2e-6, (e32, e22)
    assert not np.array_equal(y32, c["h22"])                                      # the operand rounding does something


def test_stack_reference_is_the_chain_of_layers():
    c = rg.stack_case(64, 2)
    l0, l1 = c["layers"]
    mid = oracle_np.gru(c["x"], *l0, reverse=True)
    out = oracle_np.gru(mid, *l1, reverse=False)
    full = rg.gru_stack(c["x"], c["layers"])
    assert np.abs(full - out).max() <= 1e-12
    # ragged: the first (reversed) layer of each chunk alone, then the forward layer over the chunk's own rows
    for bb, tb in enumerate(c["lens"]):
        m = oracle_np.gru(c["x"][:tb, bb:bb + 1], *l0, reverse=True)
        assert np.abs(c["h"][:tb, bb:bb + 1] - oracle_np.gru(m, *l1, reverse=False)).max() <= 1e-12
        assert np.isnan(c["h"][tb:, bb]).all()


# ------------------------------------------------------------------------------------------------------ the tables
def test_generators_are_the_distributions_they_name():
    iW, sW, sW2, b = rg.weights(96, 96, "moderate")
    assert all(a.dtype == F32 for a in (iW, sW, sW2, b))
    assert abs(sW.std() * np.sqrt(2 * 96) - 2.0) < 0.1 and abs(iW.std() * np.sqrt(192) - 1.0) < 0.05 and np.abs(sW2).max() < 1.0
    tiW, tsW, tsW2, _ = rg.weights(96, 96, "trained")
    assert np.abs(tsW2).max() == 6.0 and np.abs(tsW).max() == 6.0
    assert 50 <= np.isin(tsW2, [-6.0, 5.0, 4.5]).sum() <= 60 and abs(tiW.std() * np.sqrt(192) - 2.0) < 0.1
    x, xm = rg.inputs(96, 13, 17, 5), rg.inputs(96, 13, 17, 5, mixed=True)
    changed = np.argwhere((x != xm).any(axis=2))
    assert changed.tolist() == [[5, 1], [6, 2]]                                   # two rows of the group of steps 4 .. 7
    assert np.allclose(xm[5, 1], x[5, 1] * 1e-3) and np.allclose(xm[6, 2], x[6, 2] * 1e3)


def test_time_edges_follow_the_kernels_declared_geometry():
    """GS and R as the kernel sources state them; the time-edge set has every remainder of a group, and both sides of the first two
    ring turnovers and of the first prefetch (three groups ahead) that would pass the end."""
    for plan, want in ((1, 4), (2, 4), (3, 2)):
        gs, ring_is_two_groups = rg.declared_geometry(plan)
        assert gs == want and ring_is_two_groups, (plan, gs)
        ring = 2 * gs
        edges = set(range(1, gs + 2)) | {ring, ring + 1, 2 * ring, 2 * ring + 1, 3 * gs, 3 * gs + 1}
        assert edges <= set(rg.EDGE_T), (plan, sorted(edges - set(rg.EDGE_T)))
    assert {T % 4 for T in rg.EDGE_T} == {0, 1, 2, 3}
    sets, ahead = rg.declared_scan_period()
    assert (sets, ahead) == (4, 3)
    assert set(range(1, 10)) | {k * sets + d for k in (1, 2, 3, 4) for d in (0, 1)} <= set(rg.SCAN_T)


def test_ragged_lengths_cover_what_they_claim():
    lens = rg.ragged_lens()
    assert len(lens) == rg.RAGGED_B == 33 and max(lens) == rg.RAGGED_T and set(lens) == set(rg.RAGGED_LENGTHS)
    assert lens[-1] == 1 and lens[28:32] == (1, 1, 1, 1)                          # a four-chunk workgroup of ones; the last chunk
    for per in (4, 8, 16):
        assert 32 % per == 0                                                      # chunk 32 is alone in every plan's last workgroup
        for length in rg.RAGGED_LENGTHS:
            slots = {b % per for b in range(28) if lens[b] == length}
            assert len(slots) >= 2, (per, length)                                 # every length in at least two slot positions
        for slot in range(per):
            seen = {lens[b] for b in range(slot, 33, per)}
            assert len(seen) >= 2 and min(seen) < rg.RAGGED_T                     # every slot sees a short chunk
    for b, length in enumerate(rg.share_lens()):
        assert 1 <= length <= rg.BATCH_T
    assert 1 in rg.share_lens() and rg.BATCH_T in rg.share_lens() and len(rg.share_lens()) == rg.SHARE_B
    assert 1 in rg.STACK_LENS and max(rg.STACK_LENS) == rg.STACK_T and len(rg.STACK_LENS) == rg.STACK_B


@pytest.mark.parametrize("I,n", rg.SHAPES)
def test_every_listed_layer_case_is_admitted(I, n):
    """y22 of every (shape, regime, T) the GPU tests list, on that case's own inputs, is at most CAP / 8."""
    mine = [a for a in rg.listed_layer_cases() if a[:2] == (I, n)]
    assert len(mine) >= 2 * (len(rg.EDGE_T) + 1 + 3)
    for args in mine:
        c = rg.layer_case(*args)
        assert np.isfinite(c["h"][:1]).all()
        assert max(c["yard"].values()) <= rg.ADMIT, (args[:6], c["yard"])
        assert np.isfinite(c["x"]).all()


def test_trained_and_mixed_tables_are_subsets_of_what_was_asked():
    """Every shape has an entry, holds only lengths that were asked for, and runs `trained` at one step at least.  (What an entry leaves
    out, and the figure that rules it out, is in the table's comments; what it keeps is admitted by the test above.)"""
    for asked, table in ((rg.TRAINED_T_ASKED, rg.EDGE_T_TRAINED), (rg.MIXED_T_ASKED, rg.EDGE_T_MIXED)):
        assert set(table) == set(rg.SHAPES)
        assert all(set(ts) <= set(asked) for ts in table.values())
    assert all(1 in ts for ts in rg.EDGE_T_TRAINED.values())
    assert 0 < rg.TABLE_MARGIN < 1


def test_every_listed_scan_and_stack_case_is_admitted():
    for args in rg.listed_scan_cases():
        c = rg.scan_case(*args)
        assert max(c["yard"].values()) <= rg.ADMIT, (args[:4], c["yard"])
    for n in rg.STACK_SIZES:
        for nlayer in rg.STACK_LAYERS:
            c = rg.stack_case(n, nlayer)
            assert c["yard"]["h"] <= rg.ADMIT and c["cap"] == rg.CAP * nlayer


# ------------------------------------------------------------------- the float32 scan of csrc/recurrent.hip: recursion, cases, tables
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("act,gate", rg.OTHER_PAIRS)
def test_float64_recursion_with_other_activations_equals_the_oracles(oracle, act, gate, reverse):
    """act / gate of gru_forward against oracle_np.gru and the C oracle for every pair the float32 scan is run with; the ids are those
    of include/sloika_amd.h as sloika_amd.activation numbers them."""
    from sloika_amd import activation
    x, iW, sW, sW2, b = _small(21 + reverse)
    sW, sW2 = 0.5 * sW, 0.5 * sW2                       # (a candidate that is not squashed: keep the map from expanding)
    h = rg.gru_forward(x, iW, sW, sW2, b, reverse, act=act, gate=gate)[0]
    assert np.abs(h - oracle_np.gru(x, iW, sW, sW2, b, act=act, gate=gate, reverse=reverse)).max() <= 1e-12
    assert not np.array_equal(h, rg.gru_forward(x, iW, sW, sW2, b, reverse)[0])           # the names do something
    f = [a.astype(F32) for a in (x, iW, sW, sW2, b)]
    ref = oracle.gru(*f, act=act, gate=gate, reverse=reverse)
    # (the C oracle computes in float32: 2e-5 of the largest state, which an unsquashed candidate lets grow past 1)
    assert np.abs(rg.gru_forward(*f, reverse, act=act, gate=gate)[0] - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
    h32 = rg.gru_forward(x, iW, sW, sW2, b, reverse, None, F32, act=act, gate=gate)[0]
    assert h32.dtype == F32 and 0 < np.abs(h32 - h).max() < 2e-5 * max(1.0, np.abs(h).max())
    for name in (act, gate):
        assert rg.ACTIVATIONS[name][1] == activation.act_id(name)
    # each function where it bends: around zero, at the clip's ends, far out
    v = np.array([-30.0, -2.5, -2.0, -1e-3, 0.0, 1e-3, 2.0, 2.5, 30.0])
    for name in (act, gate):
        assert np.abs(rg.ACTIVATIONS[name][0](v) - oracle_np.ACT[name](v)).max() <= 1e-15
        assert rg.ACTIVATIONS[name][0](v.astype(F32)).dtype == F32


@pytest.mark.parametrize("reverse", [False, True])
def test_f32_scan_case_is_ragged_and_reversed_as_the_entries_document(reverse):
    """Each chunk of a ragged f32_scan_case is the case of that chunk alone over its own rows of the same vI, a reversed scan from the
    chunk's own last row; rows behind a chunk's end are MARKER; vI is the float32 rounding of the float64 projection."""
    T, lens = rg.f32_ragged_lens(4)
    c = rg.f32_scan_case(144, T, rg.F32_RAGGED_B, reverse, lens)
    assert c["grade"] == "y32" and c["h32"].dtype == F32 and c["vI"].dtype == F32 and c["zr"] is None and set(c["yard"]) == {"h"}
    assert c["yard"]["h"] == rg.chunk_errors(c["h32"], c["h"], c["lens"]).max() > 0
    for b, tb in enumerate(lens):
        alone = rg.gru_forward(None, None, c["sW"], c["sW2"], None, reverse, vI=c["vI"][:tb, b:b + 1])[0]
        assert np.abs(c["h"][:tb, b:b + 1] - alone).max() <= 1e-12
        assert np.isnan(c["h"][tb:, b]).all() and np.isnan(c["h32"][tb:, b]).all()
        if reverse and tb < T:                                                    # not the scan that starts at row T - 1
            wrong = rg.gru_forward(None, None, c["sW"], c["sW2"], None, True, vI=c["vI"][:, b:b + 1])[0]
            assert np.abs(c["h"][:tb, b:b + 1] - wrong[:tb]).max() > 1e-3
    full = rg.f32_scan_case(144, T, rg.F32_RAGGED_B, reverse, (T,) * rg.F32_RAGGED_B)
    assert np.array_equal(full["h"], rg.gru_forward(None, None, full["sW"], full["sW2"], None, reverse, vI=full["vI"])[0])
    # the same recursion as the oracle's, from the weights and inputs the case was made of
    iW, sW, sW2, b = rg.weights(rg.SCAN_INSIZE, 144, "moderate")
    plain = rg.f32_scan_case(144, 5, 3, reverse)
    x = rg.inputs(rg.SCAN_INSIZE, 5, 3, 7 * rg.SCAN_INSIZE + 3 * 144 + 5)
    assert np.array_equal(plain["vI"], (x.astype(F64) @ iW.astype(F64).T + b).astype(F32))
    assert np.array_equal(plain["sW"], sW * F32(rg.F32_RECURRENT_SCALE))
    assert np.abs(plain["h"] - oracle_np.gru(x, iW, plain["sW"], plain["sW2"], b, reverse=reverse)).max() <= 1e-6   # (vI rounded)
    small = plain.take(2)
    assert small["h32"].shape[1] == 2 and small["yard"]["h"] <= plain["yard"]["h"]


def test_f32_tables_follow_the_declared_geometry_of_recurrent_hip():
    """KB and the tile of four chunks as csrc/recurrent.hip states them; every F32_* table laid around them."""
    geo = rg.declared_f32_scan_geometry()
    assert geo == {"KB": (128, 8, 4), "tile": 4}
    widest, kb_lo, kb_hi = geo["KB"]
    assert {rg.f32_kb(n) for n in rg.F32_MFMA_SIZES if n <= widest} == {kb_lo}
    assert {rg.f32_kb(n) for n in rg.F32_MFMA_SIZES if n > widest} == {kb_hi} and set(rg.F32_T) == {kb_lo, kb_hi}
    for kb, table in rg.F32_T.items():
        assert set(table) == rg.demanded_f32_edges(kb), (kb, sorted(rg.demanded_f32_edges(kb) ^ set(table)))
        T, lengths = rg.F32_RAGGED[kb]
        assert set(lengths) == {1, kb - 1, kb, kb + 1, 2 * kb - 1, 2 * kb, 2 * kb + 1, 3 * kb, 3 * kb + 1} and T == 3 * kb + 1
    tile = geo["tile"]
    assert rg.F32_EDGE_B % tile == 1 and rg.F32_EDGE_B > 2 * tile and rg.F32_RAGGED_B % tile == 1
    assert {B % tile for B in rg.F32_BATCH_B} == set(range(tile)) and {1, tile, tile + 1, 2 * tile, 2 * tile + 1} <= set(rg.F32_BATCH_B)
    assert rg.F32_LONG_B % tile == 2
    # the instantiations of launch_gru_mfma / launch_gru_mfma144, and sizes that have none
    with open(rg.os.path.join(rg.CSRC, "recurrent.hip")) as fh:
        src = fh.read()
    sizes = {int(v) for v in rg.re.findall(r"case (\d+): return launch_gru_mfma<\1>", src)} | {int(v) for v in rg.re.findall(
        r"gru_mfma_kernel<(\d+), SLK_ACT_TANH, SLK_ACT_SIGMOID, 12>", src)}
    assert sizes == set(rg.F32_MFMA_SIZES)
    assert not set(rg.F32_GENERIC_SIZES) & sizes and max(rg.F32_GENERIC_SIZES) > max(sizes) > min(rg.F32_GENERIC_SIZES)
    assert set(rg.F32_FORCED_SIZES) <= sizes and set(rg.F32_ACT_SIZES) <= sizes and set(rg.F32_LONG_SIZES) <= sizes
    for n in rg.F32_ACT_SIZES + (144,):
        kb = rg.f32_kb(n)
        assert rg.f32_act_T(n) == (1, kb, kb + 1, 2 * kb + 1)
    assert 0 < rg.F32_RECURRENT_SCALE <= 1.0


def test_f32_ragged_sets_hold_the_tiles_they_claim():
    """B = 17 in tiles of four: three tiles of four different lengths each, the longest beside the shortest, one tile of length 1
    only, and a last tile of one chunk of length 1; every length somewhere, the ones that come twice in two slots."""
    tile = rg.declared_f32_scan_geometry()["tile"]
    for kb in rg.F32_T:
        T, lens = rg.f32_ragged_lens(kb)
        lengths = rg.F32_RAGGED[kb][1]
        assert len(lens) == rg.F32_RAGGED_B == 4 * tile + 1 and max(lens) == T and set(lens) == set(lengths)
        tiles = [lens[k:k + tile] for k in range(0, len(lens), tile)]
        assert [len(set(t)) for t in tiles] == [tile, tile, tile, 1, 1] and tiles[3] == (1,) * tile and tiles[4] == (1,)
        assert {1, T} <= set(tiles[0])                                            # a chunk that ends at once beside one that never does
        for t in tiles[:3]:
            assert min(t) < kb + 1 < max(t) or kb + 1 in t                        # lengths in different blocks of the ring
            assert len({(v - 1) // kb for v in t}) >= 3                           # ... three different last blocks per tile
        for length in lengths:
            slots = [b % tile for b in range(3 * tile) if lens[b] == length]
            assert len(slots) >= 1 and len(set(slots)) == len(slots), (kb, length, slots)
        assert sorted(v for v in lengths if lens[:3 * tile].count(v) == 2) == [1, kb + 1, T]
    assert 1 in rg.F32_GENERIC_LENS and max(rg.F32_GENERIC_LENS) == max(rg.F32_GENERIC_T) and len(rg.F32_GENERIC_LENS) == max(rg.F32_GENERIC_B)
    assert 1 in rg.F32_ACT_LENS and len(rg.F32_ACT_LENS) == rg.F32_ACT_B


def test_every_listed_f32_case_is_admitted():
    """y32 of every case the GPU tests run through the float32 scan, on that case's own inputs, is at most CAP / 8.  The time-edge,
    batch-edge and ragged sets hold every entry the geometry demands (the test above); the long and other-activation cases run at the
    lengths asked for unless their tables say otherwise."""
    listed = rg.listed_f32_cases()
    assert len(listed["edges"]) == 2 * len(rg.F32_MFMA_SIZES) * (12 + 3)
    for name, cases in listed.items():
        for args in cases:
            c = rg.f32_scan_case(*args)
            assert np.isfinite(c["vI"]).all() and c["grade"] == "y32"
            assert c["yard"]["h"] <= rg.ADMIT, (name, args[:4], args[5:], c["yard"])
    assert all(T == 100 for T in rg.F32_LONG_T.values())
    shortened = {key: ts for key, ts in rg.F32_ACT_T.items() if ts != rg.f32_act_T(key[0])}
    assert shortened == {(128, "linear"): (1, 8, 9, 15)}                          # 2 KB + 1 = 17 is not admitted there, nor is 16
    assert rg.f32_scan_case(128, 17, rg.F32_ACT_B, False, None, "linear", "sigmoid")["yard"]["h"] > rg.TABLE_MARGIN * rg.ADMIT
    T, lens = rg.f32_ragged_lens(8)
    for reverse in (False, True):
        for I, n in rg.F32_LAYER_SHAPES:
            c = rg.f32_layer_case(I, n, *rg.F32_LAYER_TB, reverse)
            assert c["grade"] == "y32" and c["yard"]["h"] <= rg.ADMIT, (I, n, c["yard"])
        for I, n, act, gate in rg.F32_NET_SCAN:
            c = rg.f32_layer_case(I, n, T, rg.F32_RAGGED_B, reverse, lens, "y22", act, gate)
            assert c["grade"] == "y22" and c["h22"].dtype == F32 and c["yard"]["h"] <= rg.ADMIT, (I, n, c["yard"])
        c = rg.f32_layer_case(*rg.F32_NET_EXACT, T, rg.F32_RAGGED_B, reverse, lens, "y32")
        assert c["yard"]["h"] <= rg.ADMIT, c["yard"]


def test_y32_of_the_float32_scan_is_the_worse_of_two_summation_orders():
    """One accumulator in the order of k against the host's BLAS: both float32, both the same recursion, and the case keeps the one
    further from float64."""
    v, W = np.random.RandomState(5).normal(size=(3, 40)).astype(F32), np.random.RandomState(6).normal(size=(7, 40)).astype(F32)
    chain = rg._product(None, "chain")(v, W)
    assert chain.dtype == F32 and chain.shape == (3, 7)
    acc = np.zeros((3, 7), F32)
    for k in range(40):
        acc = acc + v[:, k, None] * W[None, :, k]
    assert np.array_equal(chain, acc) and np.abs(chain - v.astype(F64) @ W.astype(F64).T).max() < 1e-5
    assert rg.F32_ORDERS == (None, "chain")
    c = rg.f32_scan_case(144, 4, rg.F32_ACT_B, False, None, "elu", "sigmoid")
    each = [rg.gru_forward(None, None, c["sW"], c["sW2"], None, False, None, F32, vI=c["vI"], act="elu", gate="sigmoid", order=o)[0]
            for o in rg.F32_ORDERS]
    errs = [rg.chunk_errors(h, c["h"], None).max() for h in each]
    assert c["yard"]["h"] == max(errs) and min(errs) > 0 and errs[0] != errs[1]


def test_checker_grades_a_y32_case_by_its_own_yardstick(capsys):
    c = rg.f32_scan_case(48, 9, 5, True, rg.F32_GENERIC_LENS)
    rg.check(c["h"], None, c, "self")
    rg.check(c["h32"], None, c, "y32")
    assert all(" yardstick y32 " in l for l in capsys.readouterr().out.splitlines() if l.startswith("GRUFWD "))
    got = c["h"].copy()
    got[0, 1, 5] += 3e-6                                                          # the only step of chunk 1
    with pytest.raises(AssertionError, match="chunk 1"):
        rg.check(got, None, c, "moved")
    short = rg.gru_forward(None, None, c["sW"], c["sW2"], None, True, np.array([9, 1, 4, 5, 7]), vI=c["vI"])[0]
    with pytest.raises(AssertionError, match="chunk 4"):
        rg.check(short, None, c, "short")


# ----------------------------------------------------------------------------------------------------- the checker
def _ragged(reverse):
    return rg.layer_case(48, 32, "moderate", rg.RAGGED_T, rg.RAGGED_B, reverse, rg.ragged_lens())


def test_checker_accepts_the_reference_and_the_yardstick(capsys):
    for reverse in (False, True):
        c = _ragged(reverse)
        rg.check(c["h"], c["zr"], c, "self")
        rg.check(c["h22"], c["zr22"], c, "y22")
        rg.check(c["h"].astype(F32), None, c, "rounded")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("GRUFWD ")]
    assert len(lines) == 10 and all(" ratio " in l and " chunk " in l and " bound " in l for l in lines)
    c = rg.layer_case(48, 32, "moderate", rg.BATCH_T, max(rg.BATCH_B), False)
    small = c.take(3)
    assert small["h"].shape[1] == 3 and small["B"] == 3 and c["B"] == 33
    assert small["yard"]["h"] == rg.chunk_errors(c["h22"][:, :3], c["h"][:, :3], None).max() <= c["yard"]["h"]
    rg.check(small["h"], small["zr"], small, "first three chunks")


def test_checker_rejects_one_element_moved_by_1e_5():
    c = rg.layer_case(48, 32, "moderate", 9, rg.EDGE_B, True)
    for what in ("h", "zr"):
        got = {"h": c["h"].copy(), "zr": c["zr"].copy()}
        got[what][4, 11, 7] += 1e-5
        with pytest.raises(AssertionError, match="chunk 11"):
            rg.check(got["h"], got["zr"], c, "moved")
    c = _ragged(True)
    got = c["h"].copy()
    got[0, 32, 3] -= 1e-5                                                         # the only step of the last chunk
    with pytest.raises(AssertionError, match="chunk 32"):
        rg.check(got, None, c, "moved")
    got = c["h"].copy()
    got[1, 32, 3] = 0.5                                                           # ... while behind a chunk's end nothing is compared
    rg.check(got, None, c, "behind the end")
    got = c["h"].copy()
    got[2, 5, 0] = np.nan                                                         # chunk 5 has four steps
    with pytest.raises(AssertionError, match="chunk 5"):
        rg.check(got, None, c, "nan")


@pytest.mark.parametrize("reverse", [False, True])
def test_checker_rejects_a_chunk_one_step_short(reverse):
    c = _ragged(reverse)
    for victim in (6, 10):                                                        # lengths 9 and 17
        lens = c["lens"].copy()
        lens[victim] -= 1
        h, zr = rg.gru_forward(c["x"], c["iW"], c["sW"], c["sW2"], c["b"], reverse, lens)
        with pytest.raises(AssertionError, match="chunk %d" % victim):
            rg.check(h, zr, c, "short")
        # ... also where the missing row is filled with something finite
        with pytest.raises(AssertionError, match="chunk %d" % victim):
            rg.check(np.nan_to_num(h, nan=0.0), None, c, "short, zero-filled")


def test_checker_rejects_a_reversed_chunk_started_at_the_last_row_of_the_batch():
    c = _ragged(True)
    T = rg.RAGGED_T
    for victim in (0, 9, 32):                                                     # lengths 1, 16 and 1
        tb = int(c["lens"][victim])
        assert tb < T
        h, zr = c["h"].copy(), c["zr"].copy()
        wrong = rg.gru_forward(c["x"][:, victim:victim + 1], c["iW"], c["sW"], c["sW2"], c["b"], True)      # from row T - 1
        h[:tb, victim:victim + 1], zr[:tb, victim:victim + 1] = wrong[0][:tb], wrong[1][:tb]
        with pytest.raises(AssertionError, match="chunk %d" % victim):
            rg.check(h, None, c, "started at T - 1")
        with pytest.raises(AssertionError, match="chunk %d" % victim):
            rg.check(c["h"], zr, c, "started at T - 1")


def test_checker_rejects_swapped_gates():
    c = rg.layer_case(48, 32, "moderate", 9, rg.EDGE_B, False)
    n = c["n"]
    swapped = np.concatenate([c["zr"][..., n:], c["zr"][..., :n]], axis=2)
    with pytest.raises(AssertionError, match="zr"):
        rg.check(c["h"], swapped, c, "swapped")
    with pytest.raises(AssertionError):                                           # the cap holds whatever the yardstick says
        loose = rg.Case(**c)
        loose["yard"] = {"h": 1.0, "zr": 1.0}
        rg.check(c["h"] + 3e-5, None, loose, "cap")
