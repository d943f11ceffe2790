"""Pin the oracle's chunk front end (median/MAD normalisation) against reference-generated goldens.

Reference: sloika/tools/chunkify_raw.py:172-185, sloika/maths.py:4-27, test/unit/test_maths.py:37-60.
"""
import numpy as np


def test_med_mad_kat(oracle):
    # test/unit/test_maths.py:53-60 with the default factor folded out
    x = np.array([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 1.0, 1.0], [0.0, 0.5, 0.5, 1.0]], dtype=np.float32)
    _, med, mad = oracle.med_mad_normalise(x, return_stats=True)
    assert np.allclose(med, [0.5, 0.75, 0.5])
    assert np.allclose(mad / np.float32(1.4826), [0, 0.25, 0.25])


def test_per_chunk_normalisation_bit_exact(oracle, golden_signal):
    g = golden_signal
    chunks = g["chunks_none"]
    assert chunks.shape == (5, 4000)
    assert np.array_equal(chunks.reshape(-1), g["signal"][:20000])      # raw_chunkify reshape, :172-176
    out = oracle.med_mad_normalise(chunks)
    assert np.array_equal(out, g["chunks_per_chunk"])


def test_per_read_normalisation_bit_exact(oracle, golden_signal):
    g = golden_signal
    sig = g["signal"]
    out, med, mad = oracle.med_mad_normalise(sig[None, :], return_stats=True)
    assert med[0] == g["med_mad_read"][0] and mad[0] == g["med_mad_read"][1]
    assert np.array_equal(out[0], g["read_norm"])                        # basecall.py:117-118
    # chunkify_raw.py:182-183: median/mad over the trimmed 5x4000 block
    out2 = oracle.med_mad_normalise(sig[None, :20000])
    assert np.array_equal(out2.reshape(5, 4000), g["chunks_per_read"])


# ---- the oracle against numpy's own float32 evaluation, at the shapes and on the signals tests/test_gpu_normalise.py leans on it for.
# ---- Everything by value (np.array_equal): where +0.0 and -0.0 land in a sort is unspecified in numpy and in qsort alike.
import pytest

from tests import normalise_cases as cases

LENGTHS = (1, 2, 3, 1024, 4001, 8193, 32769)


def _same_as_numpy(oracle, x):
    want, wmed, wmad = cases.numpy_med_mad_normalise(x)
    with np.errstate(all="ignore"):
        got, med, mad = oracle.med_mad_normalise(x, return_stats=True)
    assert not np.isnan(wmed).any()                                        # (a NaN median would be a case the contract excludes)
    assert np.array_equal(med, wmed) and np.array_equal(mad, wmad, equal_nan=True)
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_oracle_equals_numpy_on_every_kind(oracle, kind, n):
    _same_as_numpy(oracle, cases.make(kind, n, 3, seed=n))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("where", cases.WHERE)
def test_oracle_equals_numpy_on_constructed_groups(oracle, where, n):
    """`group` at every length (as many as 257 samples sharing their upper bits where the length allows); `mirrored` needs an even
    count, so an odd length gives its even neighbour below."""
    m = max(1, min(257, n // 3))
    x = cases.group(n, m, where, nchunk=3, seed=1)
    assert all(cases.upper16_count(row) == m for row in x)
    _same_as_numpy(oracle, x)
    ne = n - n % 2
    if ne >= 2:
        m = max(1, min(129, ne // 6))
        x = cases.mirrored(ne, m, where, nchunk=3, seed=1)
        assert np.all(np.median(x, axis=1) == 0)
        assert all(cases.upper16_count(np.abs(row)) == 2 * m for row in x)
        _same_as_numpy(oracle, x)


def test_constructed_cases_mean_what_they_say():
    """The generator's own promises: rank r on the group's first / middle / last element, and with 'last' and an even count the
    upper neighbour is the smallest filler above the group."""
    for n in (1500, 1501, 4000, 4001):
        for m in (255, 256, 257):
            for where in cases.WHERE:
                s = np.sort(cases.group(n, m, where, nchunk=2, seed=3), axis=1)
                r = (n - 1) // 2
                want = {"first": 0, "middle": m // 2, "last": m - 1}[where]
                assert np.all(s[:, r] == np.float32(64.0 + want / 1024.0))
                if where == "last":
                    assert np.all(s[:, r + 1] >= 70)
    for n in (2048, 4096):
        for m in (127, 128, 129):
            d = np.sort(np.abs(cases.mirrored(n, m, "last", nchunk=2, seed=3)), axis=1)
            assert np.all(d[:, n // 2 - 1] == np.float32(64.0 + (m - 1) / 1024.0)) and np.all(d[:, n // 2] >= 70)
    for kind in cases.KINDS:                                               # deterministic, and the seed matters
        assert np.array_equal(cases.make(kind, 257, 2, 5), cases.make(kind, 257, 2, 5), equal_nan=True)
    assert not np.array_equal(cases.make("normal", 257, 2, 5), cases.make("normal", 257, 2, 6))
    z = cases.make("signed-zeros", 4001, 1, 0)[0]
    assert np.count_nonzero((z == 0) & np.signbit(z)) > 100 and np.count_nonzero((z == 0) & ~np.signbit(z)) > 100
