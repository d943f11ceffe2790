"""oracle.map_to_sequence where reads slip over many positions, against the reference's own transducer.map_to_sequence
(tests/golden/remap_slips.npz, made by tests/golden/make_remap_slip_goldens.py), bit for bit; and the conditions that keep the
fixture -- and with it tests/test_gpu_remap_slips.py -- from going vacuous: every case's stored path shows what the case is
there for.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
import remap_slip_cases as rc          # noqa: E402  (input generators only; nothing of the reference is imported)

_FIXTURE = np.load(os.path.join(GOLD, "remap_slips.npz"))
_BUILT = {}


def slip_case(name):
    """The regenerated input of a case together with what the reference returned for it (built once and shared; no test
    writes to it)."""
    if name not in _BUILT:
        c = rc.build(name)
        c["path"] = _FIXTURE[name + "/path"]
        c["score"] = np.float32(float.fromhex(str(_FIXTURE[name + "/score_hex"])))
        c["sha256"] = str(_FIXTURE[name + "/sha256"])
        _BUILT[name] = c
    return _BUILT[name]


def test_fixture_holds_every_case():
    assert list(_FIXTURE["names"]) == rc.NAMES


@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_equals_reference(oracle, name):
    c = slip_case(name)
    assert rc.digest(c) == c["sha256"], "regenerated input differs from the one the reference saw"
    assert np.array_equal(c["seq"], _FIXTURE[name + "/seq"])
    for k in ("pi", "pf"):
        if c[k] is None:
            assert name + "/" + k not in _FIXTURE
        else:
            assert np.array_equal(c[k], _FIXTURE[name + "/" + k])
    score, path = oracle.map_to_sequence(c["ltrans"], c["seq"], c["slip"], prior_initial=c["pi"], prior_final=c["pf"])
    assert path.dtype == np.int32 and np.array_equal(path, c["path"])
    assert np.float32(score).view(np.uint32) == c["score"].view(np.uint32)


@pytest.mark.parametrize("name", rc.NAMES)
def test_stored_path_shows_what_the_case_is_for(name):
    c = slip_case(name)
    assert rc.unmet(c, c["path"], c["score"]) == []
    assert not np.isnan(c["score"]) and c["path"].min() >= 0 and c["path"].max() < len(c["seq"])
    assert (rc.jumps_of(c["path"]) >= 0).all()


def test_fixture_covers_the_long_slip_regime():
    paths = {n: slip_case(n)["path"] for n in rc.NAMES}
    jumps = np.concatenate([rc.jumps_of(p) for p in paths.values()])
    for n in rc.JUMP_LENGTHS:
        assert (jumps == n).any(), "no jump of %d anywhere in the fixture" % n
    # a batch of the device's backtrace ended by a jump out of its window on its first, second, last-but-one and last row, and
    # one ended by a jump shorter than the window
    ends = [e for p in paths.values() for e in rc.backtrace_batches(p)]
    for rows in (1, 2, rc.BATCH_ROWS - 1, rc.BATCH_ROWS):
        assert any(done == rows for done, _ in ends), rows
    assert any(jump < rc.WINDOW and done < rc.BATCH_ROWS for done, jump in ends)
    # a chain of the slip scan that outlives several of its 64 segments and is then taken by the DP
    assert any((rc.jumps_of(p) >= 3 * (((len(slip_case(n)["seq"]) - 2 + 63) >> 6) | 1)).any() for n, p in paths.items())
    # the sizes the issue names
    assert {len(p) for p in paths.values()} >= {1, 2, 3, 31, 32, 33, 34, 64, 65, 97, 2000}
    assert {len(slip_case(n)["seq"]) for n in rc.NAMES} >= {3, 4, 5, 65, 66, 67, 129, 130, 131, 194, 195, 2336, 2337, 5846}
    assert {slip_case(n)["slip"] for n in rc.NAMES} >= {0.0, 5.0, 37.25}
    assert {slip_case(n)["ltrans"].shape[1] for n in rc.NAMES} >= {65, 1025}


def test_an_exact_three_way_tie_sits_on_a_stored_path():
    """Stay, step and slip into the path's position equal at some event, recomputed here in numpy float32: the fixture pins the
    order in which the reference resolves it."""
    found = 0
    for name in ("quant_200", "quant_1000", "quant_1000_s025"):
        c = slip_case(name)
        events = rc.three_way_ties(c, c["path"])
        assert events, name
        found += len(events)
        i = events[0]
        ps = rc.forward_np(c["ltrans"], c["seq"], c["slip"], c["pi"], upto=i)
        cand = rc.candidates_np(ps, c["ltrans"][i], c["seq"], c["slip"])[:, c["path"][i]]
        assert cand[0] == cand[1] == cand[2] and np.isfinite(cand[0])
        # transducer.py:51,58: a step needs to beat the stay, a slip to beat both -- so the tie is resolved as a stay
        assert c["path"][i - 1] == c["path"][i]
    assert found >= 3


def test_numpy_forward_pass_agrees_with_the_fixture():
    """The numpy restatement the tie checks rest on returns the reference's score on the small cases."""
    for name in ("quant_200", "tie_200", "edge_small", "npos_67", "prior_both", "neginf_n65"):
        c = slip_case(name)
        final = rc.forward_np(c["ltrans"], c["seq"], c["slip"], c["pi"])
        if c["pf"] is not None:
            final = (final.astype(np.float64) + c["pf"]).astype(np.float32)
        assert final.max().view(np.uint32) == c["score"].view(np.uint32) and int(np.argmax(final)) == c["path"][-1]
