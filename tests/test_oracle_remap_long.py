"""oracle.map_to_sequence on references longer than the 5846 positions of the LDS-resident remap kernel, against the reference's own
transducer.map_to_sequence (tests/golden/remap_long.npz, made by tests/golden/make_remap_long_goldens.py), bit for bit; and the
conditions that keep the fixture -- and with it tests/test_gpu_remap_long.py -- from going vacuous.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
import remap_long_cases as lc          # noqa: E402  (input generators only; nothing of the reference is imported)

_FIXTURE = np.load(os.path.join(GOLD, "remap_long.npz"))
_BUILT = {}


def long_case(name):
    """The regenerated input of a case together with what the reference returned for it (built once and shared; no test
    writes to it)."""
    if name not in _BUILT:
        c = lc.build(name)
        c["path"] = _FIXTURE[name + "/path"]
        c["score"] = np.float32(float.fromhex(str(_FIXTURE[name + "/score_hex"])))
        c["sha256"] = str(_FIXTURE[name + "/sha256"])
        _BUILT[name] = c
    return _BUILT[name]


def test_fixture_holds_every_case():
    assert list(_FIXTURE["names"]) == lc.NAMES


@pytest.mark.parametrize("name", lc.NAMES)
def test_oracle_equals_reference(oracle, name):
    c = long_case(name)
    assert lc.digest(c) == c["sha256"], "regenerated input differs from the one the reference saw"
    assert np.array_equal(c["seq"], _FIXTURE[name + "/seq"])
    for k in ("pi", "pf"):
        if c[k] is None:
            assert name + "/" + k not in _FIXTURE
        else:
            assert np.array_equal(c[k], _FIXTURE[name + "/" + k])
    score, path = oracle.map_to_sequence(c["ltrans"], c["seq"], c["slip"], prior_initial=c["pi"], prior_final=c["pf"])
    assert path.dtype == np.int32 and np.array_equal(path, c["path"])
    assert np.float32(score).view(np.uint32) == c["score"].view(np.uint32)


@pytest.mark.parametrize("name", lc.NAMES)
def test_stored_path_shows_what_the_case_is_for(name):
    c = long_case(name)
    assert lc.unmet(c, c["path"], c["score"]) == []
    assert not np.isnan(c["score"]) and c["path"].min() >= 0 and c["path"].max() < len(c["seq"])
    assert (lc.jumps_of(c["path"]) >= 0).all()


def test_fixture_covers_what_the_tiles_need():
    cases = [long_case(n) for n in lc.NAMES]
    assert sorted(len(c["seq"]) for c in cases) == [5847, 8191, 8192, 8193, 8194, 11693, 11693, 16385]
    small = [c for c in cases if c["ltrans"].shape[1] == 65]
    assert len(small) == 7 and all(64 <= len(c["ltrans"]) <= 300 for c in small)
    assert [c["ltrans"].shape for c in cases if c["ltrans"].shape[1] != 65] == [(2000, 1025)]
    jumps = [(c, i, int(d)) for c in cases for i, d in enumerate(lc.jumps_of(c["path"])) if d >= 2]
    assert any(d >= 4096 for _, _, d in jumps)
    assert any(c["path"][i + 1] % 1024 == 1 for c, i, _ in jumps), "no jump lands on the first position after a multiple of 1024"
    assert any(c["path"][i + 1] % 1024 == 0 for c, i, _ in jumps)
    assert any(c["pi"] is not None and c["pf"] is not None for c in cases)
    assert any("far_tie" in c["needs"] and c["needs"]["far_tie"] >= 1024 for c in cases)
    assert any(not np.isfinite(c["ltrans"]).all() for c in cases)
