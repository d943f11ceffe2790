"""The forward score's fixture and host side, without a GPU: the recipes behind tests/golden/forward.npz give the bytes the
reference saw, this repository's float64 restatement (tests/forward_ref.py) reproduces the reference's scores within the fixture's
E_ref, and decode.forwards / forwards_batch / Basecaller.score_chunks refuse bad arguments before they touch a device."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import forward_cases as fc                               # noqa: E402

from tests import forward_ref                            # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "forward.npz")))


@pytest.fixture(scope="module")
def inputs(golden_decode):
    return {name: fc.build(name, golden_decode) for name in fc.NAMES}


def test_fixture_covers_the_cases(fixture):
    assert list(fixture["names"]) == fc.NAMES
    for key, name, full in fc.entries():
        assert float.fromhex(str(fixture[key + "/ref_hex"])) == float(fixture[key + "/ref"])
        assert fixture[key + "/truth"].shape == (2,)
    assert 0.0 < float(fixture["E_ref"]) < 1e-13          # a float64 recursion's distance from the exact value, not a tolerance
    # the reference's own known answers (its test/unit/test_decode.py)
    assert float(fixture["kat/free/ref"]) == -4.4275354890527474
    assert float(fixture["kat/full/ref"]) == -5.0702616325672301


def test_recipe_digests(fixture, inputs):
    """A numpy that sums (or draws) differently fails here, not on the GPU."""
    for name in fc.NAMES:
        post, seq = inputs[name]
        c = fc.CASES[name]
        assert post.shape == (c["T"], c["S"]) and str(post.dtype) == c["dtype"] and len(seq) == c["L"]
        assert np.array_equal(seq, fixture[name + "/seq"])
        assert fc.digest(post, seq) == str(fixture[name + "/sha256"]), name
        assert ((name + "/post") in fixture) == fc.stored(c)
        if fc.stored(c):
            assert post.tobytes() == fixture[name + "/post"].tobytes()
        if c["seq"] != "kat":
            assert seq.size == 0 or (seq.min() >= 0 and seq.max() <= c["S"] - 2)
    assert (inputs["sminus2"][1] == 3).any() and (inputs["sminus2_wide"][1] == 1023).any()
    assert len(set(inputs["repeat"][1])) == 1


def test_cases_sit_on_the_ownership_boundaries():
    states = sorted(c["L"] + 1 for n, c in fc.CASES.items() if n.startswith("states"))
    want = [1, 2, 63, 64, 65, 255, 256, 257]
    for ppt in (2, 4, 8, 16):
        want += [256 * ppt, 256 * ppt + 1]               # the last size of a positions-per-thread class and one step past it
    assert states == want
    for key, name, full in fc.entries():                 # `full` stays far from the underflow edge
        if full and name != "kat":                       # (the reference's own known answer is what it is)
            assert 2 * fc.CASES[name]["L"] <= fc.CASES[name]["T"]
    assert {fc.CASES[n]["S"] for n in fc.NAMES} >= {5, 1025}


def test_restatement_reproduces_the_reference(fixture, inputs):
    e_ref = float(fixture["E_ref"])
    worst = 0.0
    for key, name, full in fc.entries():
        post, seq = inputs[name]
        ref = float(fixture[key + "/ref"])
        hi, lo = (float(v) for v in fixture[key + "/truth"])
        mine = float(forward_ref.forwards(post, seq, full=full))
        d = abs(mine - ref) / max(1.0, abs(ref))
        worst = max(worst, d)
        assert d <= e_ref, (key, mine, ref)
        assert abs((ref - hi) - lo) / max(1.0, abs(hi)) <= e_ref * (1 + 1e-9), key      # E_ref is the largest of these
        assert abs(lo) <= abs(hi) * 2.0 ** -52
    print("forward_ref vs the reference: largest relative difference %.3e (E_ref %.3e)" % (worst, e_ref))


def test_restatement_structure():
    uni = np.full((3, 4), 0.25)
    assert float(forward_ref.forwards(uni, [], full=False)) == -4.1588830833596715      # the reference's value, both modes
    assert float(forward_ref.forwards(uni, [], full=True)) == -4.1588830833596715
    assert forward_ref.forwards(uni, [0, 1, 2, 0], full=True) == -np.inf                # more positions than rows
    # a blank that is not the last column: the same score with the columns rolled by one
    rs = np.random.RandomState(5)
    p = rs.dirichlet(np.ones(6), size=9)
    seq = rs.randint(0, 5, size=4)
    assert forward_ref.forwards(p, seq) == forward_ref.forwards(np.roll(p, 1, axis=1), seq + 1, blank=0)


def test_library_entry_points():
    from sloika_amd import _lib, decode
    L = _lib.lib()
    limit = L.slk_forward_score_max_positions()
    assert limit >= 4096 and decode.forward_max_positions() == limit
    bad, unsupported = _lib.SLK_ERR_INVALID_ARG, _lib.SLK_ERR_UNSUPPORTED
    p = 4096                                             # stands for a device pointer: a refused call reads and writes nothing
    assert L.slk_forward_score_batch_f32(None, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, None) == bad
    assert L.slk_forward_score_batch_f32(p, 4, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, None) == bad        # ld < nstate
    assert L.slk_forward_score_batch_f32(p, 5, p, 1, p, 5, p, p, 1, 3, 5, 0, 0.0, p, None) == bad        # blank is no column
    assert L.slk_forward_score_batch_f32(p, 5, p, 0, p, 5, p, p, 1, 3, 4, 0, 0.0, p, None) == bad        # row_step
    assert L.slk_forward_score_batch_f32(p, 5, p, 1, p, 5, p, p, 0, 3, 4, 0, 0.0, p, None) == bad        # no pairs
    assert L.slk_forward_score_batch_f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 1.0, p, None) == bad        # min_prob
    assert L.slk_forward_score_batch_f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, -1e-5, p, None) == bad
    assert L.slk_forward_score_batch_f64(p, 5, p, 1, p, 5, None, p, 1, 3, 4, 0, p, None) == bad          # positions, no sequence
    assert L.slk_forward_score_batch_f32(p, 5, p, 1, p, 5, p, p, 1, limit + 1, 4, 0, 0.0, p, None) == unsupported
    assert L.slk_forward_score_batch_f64(p, 5, p, 1, p, 5, p, p, 1, limit + 1, 4, 1, p, None) == unsupported


def test_argument_checks():
    """Every refusal comes before the device is touched (there is none here)."""
    from sloika_amd import decode
    post = np.full((6, 2, 5), 0.2, dtype=np.float32)
    limit = decode.forward_max_positions()
    with pytest.raises(ValueError, match=str(limit)):
        decode.forwards(post[:, 0], np.zeros(limit + 1, dtype=np.int64))
    with pytest.raises(ValueError, match=str(limit)):
        decode.forwards_batch(post, [[1], np.zeros(limit + 1, dtype=np.int64)])
    with pytest.raises(ValueError):
        decode.forwards(post, [1, 2])                                        # not [time, state]
    with pytest.raises(ValueError):
        decode.score(post[:, 0], [1, 5])                                     # a symbol that is no column
    with pytest.raises(ValueError):
        decode.score(post[:, 0], [-1])
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1, 2]])                                # one sequence for two pairs
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1], [2]], blank=5)
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1], [2]], lengths=[6, 7])              # more rows than the posterior has
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1], [2]], lengths=[6])
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1], [2]], min_prob=1.0)
    with pytest.raises(ValueError):
        decode.forwards_batch(post.astype(np.float64), [[1], [2]], min_prob=1e-5)    # prepare_post is float32 arithmetic
    with pytest.raises(ValueError):
        decode.forwards_batch(post[:, 0], [[1], [2]])                        # packed rows without offsets
    with pytest.raises(ValueError):
        decode.forwards_batch(post[:, 0], [[1], [2]], row_off=[0, 3])        # ... without lengths
    with pytest.raises(ValueError):
        decode.forwards_batch(post[:, 0], [[1], [2]], row_off=[0, 3, 7])     # ... past the last row
    with pytest.raises(ValueError):
        decode.forwards_batch(post, [[1], [2]], row_off=[0, 3, 6])           # offsets with the network layout


def test_score_chunks_refusals():
    from sloika_amd import layers, pipeline
    net = layers.Serial([layers.Softmax(4, 64)])
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller(net, kmer_len=3, transducer=False, fused_decode=False).score_chunks(np.zeros((2, 50), np.float32), ["ACGT"] * 2)
    bc = pipeline.Basecaller(layers.Serial([layers.Softmax(4, 65)]), kmer_len=3)
    with pytest.raises(ValueError):
        bc.score_chunks(np.zeros((2, 50), np.float32), ["ACGT"])             # one sequence for two chunks
    with pytest.raises(ValueError):
        bc.score_chunks(np.zeros((1, 50), np.float32), ["ACGNT"])            # a letter outside the alphabet
    with pytest.raises(ValueError):
        bc.score_chunks(np.zeros((1, 50), np.float32), [np.array([3, 64])])  # a state that is no 3-mer
