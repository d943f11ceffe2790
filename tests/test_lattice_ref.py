"""tests/lattice_ref.py, the numpy oracle of the lattice marginals (design/lattice_marginals.md), on the CPU: against the weight of
every path taken one by one, its row sums, its Viterbi against the oracle package's on the decode fixtures, and a lattice with a
single admissible path."""
import numpy as np
import pytest

from tests import lattice_ref as lr
from tests.conftest import decode_case_input


def _post(seed, T, S, sharp=False):
    rs = np.random.RandomState(seed)
    p = rs.dirichlet(np.ones(S) * (0.05 if sharp else 1.0), size=T).astype(np.float32)
    return (np.float32(1e-5) + np.float32(1.0 - 1e-5) * p).astype(np.float32)


@pytest.mark.parametrize("skip_pen", [0.0, 0.7, 50.0])
@pytest.mark.parametrize("nbase,T", [(2, 4), (2, 5), (3, 4)])
def test_against_every_path(nbase, T, skip_pen):
    klen = 3
    p = _post(100 * nbase + T, T, nbase ** klen + 1, sharp=(T == 5))
    gamma, logz = lr.marginals(p, klen, skip_pen, nbase)
    want, want_logz = lr.enumerate_paths(p, klen, skip_pen, nbase, dtype=np.longdouble)
    assert float(np.abs(gamma - want).max()) < 1e-12
    assert abs(float(logz - want_logz)) < 1e-12
    assert float(np.abs(gamma.sum(axis=1) - 1.0).max()) < 1e-12


@pytest.mark.parametrize("nbase,klen,T", [(4, 3, 40), (5, 3, 17), (4, 5, 30)])
def test_rows_sum_to_one(nbase, klen, T):
    p = _post(7 + klen, T, nbase ** klen + 1, sharp=True)
    for dtype in (np.float64, np.longdouble):
        gamma, logz = lr.marginals(p, klen, 0.5, nbase, dtype=dtype)
        assert gamma.dtype == dtype and (gamma >= 0).all() and np.isfinite(logz)
        assert float(np.abs(gamma.sum(axis=1) - 1.0).max()) < 1e-12


def test_long_sharp_rows_do_not_underflow():
    """800 rows whose off-path weights are near 1e-5: an unscaled float64 recursion is exactly 0 long before the end."""
    p = _post(3, 800, 65, sharp=True)
    g64, z64 = lr.marginals(p, 3, 0.0, 4)
    gld, zld = lr.marginals(p, 3, 0.0, 4, dtype=np.longdouble)
    assert np.isfinite(z64) and z64 < -800.0
    assert float(np.abs(g64 - gld).max()) < 1e-12 and abs(float(z64 - zld)) / 800 < 1e-12


def test_viterbi_is_the_oracle_packages(oracle, golden_cases, golden_decode):
    n = 0
    for case in golden_cases["decode_cases"]:
        post = decode_case_input(case, golden_decode)
        lpost = post if case["log"] else np.log(post + post.dtype.type(1e-10))
        score, path, rows = lr.viterbi(lpost, case["klen"], skip_pen=case["skip_pen"], nbase=case["nbase"])
        o_score, o_path = oracle.viterbi(post, case["klen"], skip_pen=case["skip_pen"], log=case["log"], nbase=case["nbase"])
        assert path == list(o_path) and float(score) == float(o_score), case["name"]
        # the rows: one per position, ascending from 0, and the path changes hands exactly there
        assert len(rows) == len(path) and rows[0] == 0 and all(a < b for a, b in zip(rows, rows[1:])) and rows[-1] < post.shape[0]
        n += 1
    assert n >= 3


def test_move_rows_of_a_known_path():
    """A posterior that spells out its path: states 27 (row 0), stay, 47 by step (row 2), stay, stay, 62 by step (row 5)."""
    T, klen = 6, 3
    p = np.full((T, 65), 1e-3, dtype=np.float32)
    for i, col in enumerate([1 + 27, 0, 1 + 47, 0, 0, 1 + 62]):
        p[i, col] = 0.9
    score, path, rows = lr.viterbi(np.log(p + np.float32(1e-10)), klen)
    assert path == [27, 47, 62] and rows == [0, 2, 5]
    gamma, _ = lr.marginals(p, klen)
    conf = lr.confidence(gamma, path, rows)
    assert conf.shape == (3,) and (conf > 0.9).all() and (conf <= 1.0).all()
    assert conf[1] == gamma[2:5, 47].max()


def test_one_admissible_path_has_confidence_one():
    """A one-hot posterior with min_prob = 0: every other path weighs exactly 0, every factor of the one left is exactly 1."""
    klen, nbase = 3, 4
    N = nbase ** klen
    seq = [0, 1, 2, 3, 0, 2, 1, 3]                          # ACGTAGCT: no k-mer follows its predecessor by a skip as well
    states = [seq[i] * 16 + seq[i + 1] * 4 + seq[i + 2] for i in range(len(seq) - 2)]
    for q, s in zip(states, states[1:]):
        assert s // nbase == q % (N // nbase) and s // nbase ** 2 != q % (N // nbase ** 2) and s != q
    cols = [1 + states[0], 0, 0]
    for s in states[1:]:
        cols += [1 + s, 0]
    p = np.zeros((len(cols), N + 1), dtype=np.float32)
    p[np.arange(len(cols)), cols] = 1.0
    score, path, rows = lr.viterbi(np.log(p + np.float32(1e-10)), klen)
    assert path == states
    for dtype in (np.float64, np.longdouble):
        gamma, logz = lr.marginals(p, klen, 0.0, nbase, dtype=dtype)
        assert logz == 0.0
        conf = lr.confidence(gamma, path, rows)
        assert (conf == 1.0).all()
        assert (gamma.sum(axis=1) == 1.0).all()
