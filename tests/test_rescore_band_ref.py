"""The CPU model of banded rescoring (tests/rescore_band_ref.py, written from design/rescore_band.md) against the dense model it
extends, and, from the shapes alone, that the cases of tests/test_gpu_rescore_band.py reach the tiers of csrc/rescore_band.hip they
are meant for.  No GPU."""
import math

import numpy as np
import pytest

from tests import rescore_ref as rr
from tests import rescore_band_ref as rb

E_REF = 3.219e-15


def close(a, b, k=4.0):
    if a != a or b != b:
        return a != a and b != b
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= k * E_REF * max(1.0, abs(b))


def planted(T=300, L=120, S=17, seed=3):
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, S - 1, size=L)
    post = rng.uniform(size=(T, S)) * rng.uniform(size=(T, S))
    rows = np.sort(rng.choice(T, size=L, replace=False))
    post[rows, seq] += 1.0
    post[:, -1] += 0.3
    post /= post.sum(axis=1, keepdims=True)
    edits = [(0, 1, [1]), (0, 0, [2]), (L, 0, [3]), (L - 1, 1, []), (L // 2, 1, [int(seq[L // 2])]), (30, 2, [4, 5, 6, 7, 8, 9, 10, 11]),
             (60, 0, [1, 2]), (90, 3, [5]), (17, 1, []), (101, 1, [0, 0, 0])]
    return post, seq, edits, rb.center_from_rows(rows, T)


def test_a_band_that_holds_every_state_has_the_dense_bits():
    for post, seq, edits in rr.tiny_cases() + rr.wide_cases():
        T, L = post.shape[0], len(seq)
        want = rr.rescore(post, seq, edits)
        for W in (L + 1, rb.width_for(L)):
            got = rb.rescore(post, seq, edits, rb.zero_band(T), W)
            assert np.array_equal(np.array([want[0]] + want[1]), np.array([got[0]] + got[1]), equal_nan=True), (T, L, W)


def test_nested_bands_never_exceed_the_dense_model():
    """The issue's experiment: 300 rows x 17 columns x 120 positions, 10 edits, bands of 8 .. 128 states round the planted path."""
    post, seq, edits, center = planted()
    T, L = post.shape[0], len(seq)
    dense = rr.rescore(post, seq, edits)
    dense = [dense[0]] + dense[1]
    prev, gaps = None, {}
    for W in (8, 16, 32, 128):
        lo = rb.band_lo(center, L, W)
        assert rb.valid_band(lo, T, L, W)
        got = rb.rescore(post, seq, edits, lo, W)
        got = [got[0]] + got[1]
        for i, (g, d) in enumerate(zip(got, dense)):
            slack = 4 * E_REF * max(1.0, abs(d))
            assert g <= d + slack, (W, i)
            assert prev is None or prev[i] <= g + slack, (W, i)
        gaps[W] = max(d - g for g, d in zip(got, dense))
        prev = got
    # what a band loses falls fast with its width: whole units at 8 states, nothing that float64 can tell at 128
    assert gaps[8] > 1e-6 and gaps[32] < 1e-6 and gaps[128] <= 4 * E_REF * abs(dense[0])


def test_the_vector_form_is_the_model():
    """evaluate() in float64 is rescore() but for the order of the row totals; in np.longdouble it is the truth."""
    post, seq, edits, center = planted()
    lo = rb.band_lo(center, len(seq), 32)
    want = rb.rescore(post, seq, edits, lo, 32)
    for ld in (np.float64, np.longdouble):
        s, ll = rb.evaluate(post, seq, edits, lo, 32, -1, ld)
        assert close(float(s), want[0], 1.0) and all(close(float(a), b, 1.0) for a, b in zip(ll, want[1]))
    post, seq, edits, lo = rb.ring_case(5, 600, 256, lossy=True)
    want = rb.rescore(post, seq, edits, lo, 256)
    s, ll = rb.truth(post, seq, edits, lo, 256)
    assert close(float(s), want[0], 1.0) and all(close(float(a), b, 1.0) for a, b in zip(ll, want[1]))


def test_an_empty_range_scores_minus_infinity():
    n = 0
    for S, L, W in rb.RING:
        for lossy in (False, True):
            post, seq, edits, lo = rb.ring_case(S, L, W, lossy=lossy)
            T = post.shape[0]
            assert rb.valid_band(lo, T, L, W)
            score, ll = rb.rescore(post, seq, edits, lo, W)
            for (a, d, new), v in zip(edits, ll):
                t0, t1 = rb.rows_of(lo, W, a)
                tend = rb.rows_of(lo, W, a + d + 1)[1] if a + d < L else T
                if t0 > t1 or (a + d < L and tend <= t0):
                    assert v == -math.inf, (L, W, a, d)
                    n += 1
            assert sum(math.isfinite(v) for v in ll) >= 5
    assert n >= 6
    # an invalid band: everything NaN
    post, seq, edits, lo = rb.ring_case(5, 600, 256)
    for bad in (np.maximum(lo, 1), -lo, lo[::-1].copy(), np.minimum(lo, 600 - 256)):
        s, ll = rb.rescore(post, seq, edits[:3], bad, 256)
        assert s != s and all(v != v for v in ll)


@pytest.mark.parametrize("S,L,W", rb.RING)
def test_ring_cases_reach_their_tiers(S, L, W):
    """From the shapes alone: the ring wraps more than twice, a band step crosses a thread, a wave and the ring's end, steps come in
    consecutive rows and fs_ahead rows apart, every step of the list occurs, and candidates sit on the band's edges."""
    ppt, D = rb.ppt_of(W), rb.ahead_of(W)
    assert (L + 1) / W > 2 and W == 256 * ppt and D == (4 if ppt <= 4 else 2)
    for lossy in (False, True):
        post, seq, edits, lo = rb.ring_case(S, L, W, lossy=lossy)
        T = post.shape[0]
        facts = rb.ring_facts(lo, W, L)
        assert facts["thread"] and facts["wave"] and facts["ring"] and facts["consecutive"]
        want = [s for s in rb.ring_steps(W) if lossy or s < W]
        assert set(want) <= set(facts["steps"])
        rows = facts["step_rows"]
        assert any(b - a == 1 for a, b in zip(rows, rows[1:])) and any(b - a == D for a, b in zip(rows, rows[1:]))
        lo = [int(v) for v in lo]
        first = [rb.rows_of(lo, W, a)[0] for a, _, _ in edits]
        last = [rb.rows_of(lo, W, a)[1] for a, _, _ in edits]
        assert any(a == lo[t] for (a, _, _), t in zip(edits, last) if 0 <= t <= T)              # a == lo[t] in a's last row
        assert any(a == lo[t] + W - 1 for (a, _, _), t in zip(edits, first) if 0 <= t <= T)      # a == lo[t] + W - 1 in a's first row
        assert any(any(a + d + 1 == lo[t] + W for t in range(T + 1)) for a, d, _ in edits)       # one past the band
        if lossy:                                                 # (a step above W + 1 skips both columns of an edit)
            assert any(rb.rows_of(lo, W, a)[0] > rb.rows_of(lo, W, a + d + 1)[1] for a, d, _ in edits if a + d < L)
            assert any(rb.rows_of(lo, W, a)[0] > rb.rows_of(lo, W, a)[1] for a, d, _ in edits)
        assert any(a == 0 for a, _, _ in edits) and any(a + d == L for a, d, _ in edits)
        assert {len(n) for _, _, n in edits} >= {0, 1, 8}
    # the mass itself goes round the ring in the diagonal pairs and the long one
    assert rb.ahead_of(256) == 4 and [c[0].shape[0] for c in rb.few_rows_cases()] == [0, 1, 2, 3, 4, 5]


def test_dense_tie_cases_take_the_dense_kernel_s_ownership():
    for L in (255, 256, 511, 512):
        assert rb.width_for(L) == 256 * rr.ppt_of(L)
    assert all(rb.width_for(len(c[1])) == 256 for c in rr.tiny_cases())


def test_polish_planted_long_returns_the_truth_with_the_band():
    """T = 3 000, L = 1 000 k-mers, three reads, W = 256: one round takes the three planted edits, the truth comes back, and the centre
    lines of the second round are the shifted ones."""
    truth, draft, posts, centers = rb.planted_long()
    assert len(rr.states_of(truth, 3)) == 1000 and posts[0].shape == (3000, 65)
    text, applied, rounds, total = rb.polish(posts, draft, 3, centers, 256)
    assert text == truth and rounds == 1
    assert sorted((a[1], a[2]) for a in applied) == [('del', 848), ('ins', 520), ('sub', 200)]
    assert min(a[4] for a in applied) > 5.0
    pos = sorted(a[2] for a in applied)
    assert min(b - a for a, b in zip(pos, pos[1:])) > 300


def test_shift_center():
    c = np.array([0, 1, 5, 5, 6, 9, 12])
    assert list(rb.shift_center(c, [(5, 1, 0)])) == [0, 1, 5, 5, 5, 8, 11]
    assert list(rb.shift_center(c, [(5, 0, 1), (0, 2, 2), (9, 3, 1)])) == [0, 1, 5, 5, 7, 10, 11]
    assert list(rb.shift_center(c, [])) == list(c)
