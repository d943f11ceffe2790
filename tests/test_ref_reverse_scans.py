"""tests/ref_reverse_scans.py on the CPU: the three float64 references against the training oracle (oracle/oracle_train.py, itself
pinned to the reference's own automatic differentiation and to finite differences) on one-layer networks, so that they are no
third opinion of unknown standing; and the properties of the generated inputs and yardsticks that the GPU tests lean on."""
import numpy as np
import pytest

from oracle import oracle_train as ot
from tests import ref_reverse_scans as rr


def _loss_head(rs, out, nstate):
    """Softmax layer + weighted cross-entropy of train_network.py:128-136 on top of a layer output out:[T][B][n], written out:
    returns the softmax spec, labels, weights and dL/dout."""
    T, B, n = out.shape
    W, b = rs.normal(size=(nstate, n)) * 0.5, rs.normal(size=nstate) * 0.5
    labels, weights = rs.randint(0, nstate, size=(T, B)), rs.uniform(0.5, 1.5, size=(T, B))
    logits = out @ W.T + b
    p = np.exp(logits - logits.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    onehot = np.eye(nstate)[labels]
    dlogits = (weights / (T * B))[:, :, None] * (p - onehot)       # min_prob = 0, drop = 0
    return {"type": "softmax", "W": W, "b": b}, labels, weights, dlogits @ W


def _close(got, want):
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("reverse", [False, True])
def test_gru_reference_vs_training_oracle(reverse):
    rs = np.random.RandomState(31 + reverse)
    T, B, I, n = 13, 4, 5, 7
    iW, sW, sW2, b = (rs.normal(size=s) * 0.8 for s in ((3 * n, I), (2 * n, n), (n, n), (3 * n,)))
    x = rs.normal(size=(T, B, I))
    # the forward pass in scan order (layers.py:1010-1021)
    xs = x[::-1] if reverse else x
    h = np.zeros((T + 1, B, n))
    z, r, c = (np.zeros((T, B, n)) for _ in range(3))
    for s in range(T):
        vI, vS = xs[s] @ iW.T + b, h[s] @ sW.T
        z[s], r[s] = rr.sigmoid(vI[:, :n] + vS[:, :n]), rr.sigmoid(vI[:, n:2 * n] + vS[:, n:])
        c[s] = np.tanh(vI[:, 2 * n:] + (r[s] * h[s]) @ sW2.T)
        h[s + 1] = z[s] * h[s] + (1 - z[s]) * c[s]
    tm = lambda a: (a[::-1] if reverse else a).reshape(T * B, -1)   # scan order -> rows in time order
    out = (h[1:][::-1] if reverse else h[1:])
    head, labels, weights, dout = _loss_head(rs, out, 6)
    da, rh = rr.gru_reverse_scan(dout.reshape(T * B, n), tm(z), tm(r), tm(c), tm(h[:-1]), sW, sW2, T, B, reverse)
    gru = {"type": "GRU", "iW": iW, "sW": sW, "sW2": sW2, "b": b, "activation": "tanh", "gate": "sigmoid"}
    spec = {"type": "serial", "sublayers": [{"type": "reverse", "sublayer": gru} if reverse else gru, head]}
    _, _, grads = ot.loss_and_grads(spec, x, labels, weights)
    _close(da.T @ x.reshape(T * B, I), grads[0])
    _close(da[:, :2 * n].T @ tm(h[:-1]), grads[1])
    _close(da[:, 2 * n:].T @ rh, grads[2])
    _close(da.sum(axis=0), grads[3])
    np.testing.assert_array_equal(rh, tm(r) * tm(h[:-1]))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("peepholes", [True, False])
def test_lstm_references_vs_training_oracle(reverse, peepholes):
    rs = np.random.RandomState(41 + reverse + 2 * peepholes)
    T, B, I, n = 11, 3, 4, 6
    iW, sW, b = (rs.normal(size=s) * 0.8 for s in ((4 * n, I), (4 * n, n), (4 * n,)))
    peep = rs.normal(size=(3, n)) * 0.8 if peepholes else None
    pp = np.zeros((3, n)) if peep is None else peep
    x = rs.normal(size=(T, B, I))
    xs = x[::-1] if reverse else x
    # the forward pass in scan order (layers.py:677-697): what it feeds its gates with, and what it makes of it
    sm, outs, cells, gates = np.zeros((T, B, 4 * n)), np.zeros((T + 1, B, n)), np.zeros((T + 1, B, n)), np.zeros((T, B, n, 4))
    for s in range(T):
        sm[s] = xs[s] @ iW.T + outs[s] @ sW.T + b
        v = sm[s].reshape(B, n, 4)
        g, i, f = np.tanh(v[:, :, 0]), rr.sigmoid(v[:, :, 1] + cells[s] * pp[0]), rr.sigmoid(v[:, :, 2] + cells[s] * pp[1])
        cells[s + 1] = cells[s] * f + g * i
        o = rr.sigmoid(v[:, :, 3] + cells[s + 1] * pp[2])
        gates[s] = np.stack([g, i, f, o], axis=2)
        outs[s + 1] = np.tanh(cells[s + 1]) * o
    tm = lambda a: (a[::-1] if reverse else a).reshape(T * B, -1)
    g_ref, c_ref = rr.lstm_cell_scan(tm(sm), peep, T, B, reverse)
    np.testing.assert_allclose(g_ref, tm(gates.reshape(T, B, 4 * n)), rtol=0, atol=1e-15)
    np.testing.assert_allclose(c_ref, tm(cells[1:]), rtol=0, atol=1e-15)
    out = outs[1:][::-1] if reverse else outs[1:]
    head, labels, weights, dout = _loss_head(rs, out, 5)
    dsum, dpeep = rr.lstm_reverse_scan(dout.reshape(T * B, n), g_ref, c_ref, sW, peep, T, B, reverse)
    lstm = {"type": "LSTM", "iW": iW, "sW": sW, "b": b, "p": peep, "activation": "tanh", "gate": "sigmoid"}
    spec = {"type": "serial", "sublayers": [{"type": "reverse", "sublayer": lstm} if reverse else lstm, head]}
    _, _, grads = ot.loss_and_grads(spec, x, labels, weights)
    _close(dsum.T @ x.reshape(T * B, I), grads[0])
    _close(dsum.T @ tm(outs[:-1]), grads[1])
    _close(dsum.sum(axis=0), grads[2])
    if peepholes:
        _close(dpeep.sum(axis=0), grads[3])
    else:
        # without peepholes the per-chunk sums are still formed (sum_t di' c_{t-1}, ...); they equal those of a zero-peephole layer
        assert np.array_equal(dpeep, rr.lstm_reverse_scan(dout.reshape(T * B, n), g_ref, c_ref, sW, np.zeros((3, n)), T, B, reverse)[1])


def test_round22_keeps_22_bits_of_the_row_top():
    rs = np.random.RandomState(5)
    a = (rs.normal(size=(40, 64)) * 10.0 ** rs.uniform(-30, 30, size=(40, 1))).astype(np.float32)
    a[3] = 0.0
    for axis in (0, 1):
        v = a if axis == 1 else a.T
        got = rr.round22(v, axis).astype(np.float64)
        top = np.abs(v).max(axis=axis, keepdims=True).astype(np.float64)
        err = np.abs(got - v)
        assert (err <= 2.0 ** -22 * np.abs(v) + 2.0 ** -24 * top).all()
        assert (err > 2.0 ** -25 * np.abs(v)).mean() > 0.2                # ... and it IS coarser than float32
    assert not rr.round22(a, 1)[3].any()
    assert np.array_equal(rr.round22(np.array([[1.0, -0.5, 1.5]], np.float32), 1), np.array([[1.0, -0.5, 1.5]], np.float32))


@pytest.mark.parametrize("n,T,B", [(16, 23, 9), (64, 61, 5), (128, 3, 261), (32, 2, 3), (16, 1, 5)])
def test_saturated_regime_saturates(n, T, B):
    """Regime 2 really saturates, at a measurable share where the case is large enough to speak of shares.  (The GPU tests assert
    the same on the very inputs of each of their cases: the generator, seeds and shapes are theirs.)"""
    for reverse in (False, True):
        g, l = rr.gru_case(n + T, T, B, n, "saturated", reverse), rr.lstm_case(n + T, T, B, n, "saturated", reverse)
        rr.assert_gru_saturated(g)
        rr.assert_gru_saturated(rr.gru_case(n + T, T, B, n, rr.NOISY_H, reverse))
        rr.assert_lstm_saturated(l)
        if T * B * n > 1000:
            z, gt = g["z"], l["gates"]
            assert (z == 1.0).mean() > 0.03 and ((z > 1.0 - 1e-6) & (z < 1.0)).mean() > 0.01
            assert (gt[:, 2::4] == 1.0).mean() > 0.03 and (gt[:, 3::4] == 1.0).mean() > 0.03
            assert (np.abs(gt[:, 0::4]) == 1.0).mean() > 0.3                  # and candidates at tanh's ends


@pytest.mark.parametrize("regime", rr.REGIMES + (rr.NOISY_H,))
@pytest.mark.parametrize("reverse", [False, True])
def test_yardsticks_stay_below_the_suites_caps(regime, reverse):
    """The yardsticks themselves, on the CPU, Gru and Lstm, n = 32, (T, B) = (23, 9): float32 arithmetic below 2e-6 of a chunk's top
    and 22-bit operands below 1e-5 in every regime with moderate weights and an exact h (saturation costs the recovered candidate
    nothing in this normalisation); below the suite's 1e-4 with trained magnitudes and with a noisy h; an all-zero chunk stays
    exactly zero.  (No order between y32 and y22 is asserted: 22-bit operands often come out no worse than float32.)"""
    T, B, n = 23, 9, 32
    # trained: errors add up over steps that expand the gradient, so the suite's cap for large weights; NOISY_H: h is off by 1e-5
    # and c = (h - z h') / (1 - z) with it
    c32, c22 = (1e-4, 1e-4) if regime in ("trained", rr.NOISY_H) else (2e-6, 1e-5)
    g = rr.gru_case(7, T, B, n, regime, reverse)
    ref, _ = rr.gru_reverse_scan(g["dy"], g["z"], g["r"], g["c"], g["h_prev"], g["sW"], g["sW2"], T, B, reverse)
    assert np.isfinite(ref).all() and np.abs(ref).max() < 1e30
    y32 = rr.chunk_error(rr.gru_reverse_scan_f32(g["dy"], g["z"], g["r"], g["h"], g["h_prev"], g["sW"], g["sW2"], T, B, reverse)[0], ref, T, B)
    y22 = rr.chunk_error(rr.gru_reverse_scan_f32(g["dy"], g["z"], g["r"], g["h"], g["h_prev"], g["sW"], g["sW2"], T, B, reverse, 22)[0], ref, T, B)
    assert y32.max() < c32 and y22.max() < c22, (y32.max(), y22.max())
    l = rr.lstm_case(7, T, B, n, regime, reverse)
    ref, refp = rr.lstm_reverse_scan(l["dy"], l["gates"], l["cell"], l["sW"], l["peep"], T, B, reverse)
    assert np.isfinite(ref).all() and np.abs(ref).max() < 1e30
    for bits, cap in ((None, c32), (22, c22)):
        y, yp = rr.lstm_reverse_scan(l["dy"], l["gates"], l["cell"], l["sW"], l["peep"], T, B, reverse, np.float32, bits)
        assert rr.chunk_error(y, ref, T, B).max() < cap, (bits, rr.chunk_error(y, ref, T, B).max())
        assert rr.chunk_error(yp, refp, 1, B).max() < cap
        if regime.startswith("mixed"):
            assert not y.reshape(T, B, -1)[:, 3].any() and not yp[3].any()
    if regime.startswith("mixed"):
        assert not ref.reshape(T, B, -1)[:, 3].any() and not refp[3].any()
