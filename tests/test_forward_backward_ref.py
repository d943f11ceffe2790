"""The forward-backward oracle of the GPU tests (tests/forward_backward_ref.py) pinned to the forward score it extends, without a
GPU: its score is tests/forward_ref.py's, its occupancies are p times the derivative of that score by p, every row sums to 1, and a
`full` pair with more positions than rows has none; and what the C entries decide on the host: the exact workspace and the
refusals.  (design/forward_backward.md)"""
import os
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import forward_cases as fc                               # noqa: E402

from tests import forward_backward_ref as fbr            # noqa: E402
from tests import forward_ref                            # noqa: E402

LD = np.longdouble                                       # extended precision (eps 1.08e-19), as the forward fixture's generator needs

T, S, L = 40, 5, 12


@pytest.fixture(scope="module")
def pair():
    return fc.make_post(4101, T, S, "float64"), fc.make_seq(4101, S, L, "random")


def test_score_is_the_forward_score(pair):
    e_ref = float(np.load(os.path.join(GOLDEN, "forward.npz"))["E_ref"])
    post, seq = pair
    for name in ("rows3", "states65", "repeat", "sminus2", "wide_small"):
        p, q = fc.build(name)
        for full in fc.CASES[name]["modes"]:
            mine = float(fbr.forwards_backwards(p, q, full=full)[0])
            ref = float(forward_ref.forwards(p, q, full=full))
            assert abs(mine - ref) / max(1.0, abs(ref)) <= e_ref, (name, full, mine, ref)
    for full in (False, True):
        assert abs(float(fbr.forwards_backwards(post, seq, full=full)[0]) - float(forward_ref.forwards(post, seq, full=full))) <= e_ref * 60


def test_occupancy_is_p_times_the_scores_derivative(pair):
    post, seq = pair
    h = LD(1e-9)
    worst = 0.0
    for full in (False, True):
        occ = fbr.forwards_backwards(post, seq, full=full, dtype=LD)[1]
        for t in (0, 17, T - 1):
            for c in range(S):
                up, down = post.astype(LD), post.astype(LD)
                up[t, c] += h
                down[t, c] -= h
                slope = (fbr.forwards_backwards(up, seq, full=full, dtype=LD)[0]
                         - fbr.forwards_backwards(down, seq, full=full, dtype=LD)[0]) / (2 * h)
                d = float(abs(occ[t, c] - LD(post[t, c]) * slope))
                worst = max(worst, d)
                assert d <= 1e-7, (full, t, c, d)
    print("occ against central differences of the score: largest difference %.3e" % worst)


def test_rows_sum_to_one_and_float64_is_close_to_extended(pair):
    post, seq = pair
    eps = np.finfo(np.float64).eps
    for full in (False, True):
        score, occ, row, prob, gap = fbr.forwards_backwards(post, seq, full=full, gaps=True)
        assert np.isfinite(score) and occ.dtype == np.float64
        assert np.abs(occ.sum(axis=1) - 1.0).max() <= 8 * eps
        truth = fbr.forwards_backwards(post, seq, full=full, dtype=LD)
        assert float(np.abs(occ - truth[1]).max()) <= 8 * eps
        assert np.array_equal(row, truth[2]) and float(np.abs(prob - truth[3]).max()) <= 8 * eps
        assert (row >= 0).all() and (prob > 0).all() and float(gap.min()) > 1e-3
        # a position is emitted where the oracle says: the reported value is that row's
        assert occ[row, seq].min() >= prob.min() * (1 - 1e-12)


def test_same_symbol_and_blank_symbol_add_up():
    post = fc.make_post(4102, 9, 5, "float64")
    _, occ, _, prob = fbr.forwards_backwards(post, [2, 2, 2], blank=0)
    assert np.allclose(occ.sum(axis=1), 1.0, atol=1e-15) and (occ[:, [1, 3, 4]] == 0).all()
    _, occ, row, prob = fbr.forwards_backwards(post, [0, 3], blank=0)           # a symbol equal to the blank adds to that column
    assert np.allclose(occ.sum(axis=1), 1.0, atol=1e-15) and (occ[:, [1, 2, 4]] == 0).all()


def test_degenerate_pairs():
    post = fc.make_post(4103, 4, 5, "float64")
    score, occ, row, prob = fbr.forwards_backwards(post, [0, 1, 2, 3, 0], full=True)       # more positions than rows
    assert score == -np.inf and not occ.any() and (row == -1).all() and not prob.any()
    score, occ, row, prob = fbr.forwards_backwards(post, [], full=True)                    # no positions: every row stays
    assert np.array_equal(occ[:, -1], np.ones(4)) and not occ[:, :-1].any() and row.size == 0
    score, occ, row, prob = fbr.forwards_backwards(post[:0], [1, 2])                       # no rows
    assert score == 0.0 and occ.shape == (0, 5) and (row == -1).all() and not prob.any()
    # two identical consecutive rows, free mode: the tie goes to the lower row
    tie = np.repeat(np.array([[0.1, 0.6, 0.1, 0.1, 0.1]]), 2, axis=0)
    _, _, row, prob, gap = fbr.forwards_backwards(tie, [1], gaps=True)
    assert row[0] == 0 and gap[0] == 0.0


def test_c_entry_host_side():
    """What the C entries decide on the host, before they touch a device: the exact workspace and the refusals."""
    import ctypes
    from sloika_amd import _lib, build
    build.build()
    L = _lib.lib()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                  # noqa: E731
    limit = L.slk_forward_score_max_positions()
    nrow = np.array([10, 0, 3, 7, 5, -1], np.int32)
    npos = [0, 4, 256, 2047, limit, 3]                      # ppt 1, (no rows), 2, 8, 32, (refused on the device)
    pos = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    want = 256 + 8 * 256 * (10 * 1 + 3 * 2 + 7 * 8 + 5 * 32)
    assert L.slk_forward_backward_workspace_bytes(6, ptr(nrow), ptr(pos)) == want
    assert L.slk_forward_backward_workspace_bytes(0, ptr(nrow), ptr(pos)) == 0
    assert L.slk_forward_backward_workspace_bytes(40, ptr(np.zeros(40, np.int32)), ptr(np.zeros(41, np.int64))) == 512   # the table alone
    p = ctypes.c_void_p(256)
    bad, unsupported, short = _lib.SLK_ERR_INVALID_ARG, _lib.SLK_ERR_UNSUPPORTED, _lib.SLK_ERR_WORKSPACE
    f32 = lambda *a: L.slk_forward_backward_batch_f32(*a)                              # noqa: E731
    assert f32(None, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, p, 5, p, p, p, 4096, None) == bad
    assert f32(p, 4, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, p, 5, p, p, p, 4096, None) == bad          # ld < nstate
    assert f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, p, 4, p, p, p, 4096, None) == bad          # occ_ld < nstate
    assert f32(p, 5, p, 1, p, 5, p, p, 1, 3, 5, 0, 0.0, p, p, 5, p, p, p, 4096, None) == bad          # blank is no column
    assert f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 1.0, p, p, 5, p, p, p, 4096, None) == bad          # min_prob
    assert f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, None, p, 5, p, p, p, 4096, None) == bad       # no score
    assert f32(p, 5, p, 1, p, 5, p, p, 1, limit + 1, 4, 0, 0.0, p, p, 5, p, p, p, 4096, None) == unsupported
    assert f32(p, 8193, p, 1, p, 8193, p, p, 1, 3, 4, 0, 0.0, p, p, 8193, p, p, p, 4096, None) == unsupported
    assert f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, None, 0, None, None, None, 4096, None) == short    # no workspace
    assert L.slk_forward_backward_batch_f64(p, 5, p, 1, p, 5, None, p, 1, 3, 4, 1, p, p, 5, p, p, p, 4096, None) == bad    # positions, no sequence
