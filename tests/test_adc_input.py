"""int16 ADC input (slk_adc_to_pa_i16 and the host side of `scaling=`) without a GPU: the C ABI entry point and its argument checks,
the scaling helper (batch.adc_scaling) against the arithmetic of fast5.Fast5.get_read, and Fast5.scaling()."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_READS = os.path.join("/root/reference", "data", "reads")
have_ref = os.path.isdir(REF_READS)


@pytest.fixture(scope="module")
def built():
    from sloika_amd import build
    return build.build()


def test_entry_point_is_declared_and_bound(built):
    from sloika_amd import _lib
    with open(os.path.join(ROOT, "include", "sloika_amd.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert re.search(r"\bslk_adc_to_pa_i16\s*\(", text)
    res, args = _lib.PROTOTYPES["slk_adc_to_pa_i16"]
    assert res is ctypes.c_int and len(args) == 11
    assert hasattr(ctypes.CDLL(built), "slk_adc_to_pa_i16")


def test_argument_checks_return_before_any_hip_call(built):
    """Refused arguments come back as SLK_ERR_INVALID_ARG with no device involved (this box may have none)."""
    from sloika_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    full = [p, p, p, p, p, p, 1, 8, p, p, None]
    for k in (0, 1, 2, 3, 4, 5, 8):                      # every array but the nullable flags
        a = list(full)
        a[k] = None
        assert L.slk_adc_to_pa_i16(*a) == _lib.SLK_ERR_INVALID_ARG, k
    a = list(full)
    a[6] = -1                                            # nread < 0
    assert L.slk_adc_to_pa_i16(*a) == _lib.SLK_ERR_INVALID_ARG
    a = list(full)
    a[7] = -4                                            # a negative length (max_stride)
    assert L.slk_adc_to_pa_i16(*a) == _lib.SLK_ERR_INVALID_ARG
    a = list(full)
    a[6] = 0                                             # nothing to do: no launch
    assert L.slk_adc_to_pa_i16(*a) == _lib.SLK_OK


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_scaling_helper_matches_fast5_arithmetic():
    from sloika_amd import batch
    g = np.load(os.path.join(GOLDEN, "reads.npz"))
    reads, trip = [], []
    for n in (3, 5):
        dig, off, rng, _rate = (float(v) for v in g["meta_%d" % n])
        reads.append(g["adc_%d" % n])
        trip.append((off, rng, dig))
    off, sc = batch.adc_scaling(reads, trip)
    assert off.dtype == np.float64 and sc.dtype == np.float64
    assert np.array_equal(_bits(off), _bits([t[0] for t in trip]))
    assert np.array_equal(_bits(sc), _bits([t[1] / t[2] for t in trip]))          # float(range) / float(digitisation)
    # random triples, including values whose quotient rounds
    rs = np.random.RandomState(3)
    n = 500
    t = np.stack([rs.uniform(-300, 300, n), rs.uniform(100, 3000, n), rs.choice([2048.0, 8192.0, 8191.0, 3.0], n)], axis=1)
    sigs = [np.zeros(rs.randint(0, 5), dtype=np.int16) for _ in range(n)]
    off, sc = batch.adc_scaling(sigs, t)
    assert np.array_equal(_bits(off), _bits(t[:, 0]))
    assert np.array_equal(_bits(sc), _bits([float(r) / float(d) for r, d in t[:, 1:]]))
    # digitisation 0 is no error on the host: the scale is infinite and the kernel flags the read
    _, sc0 = batch.adc_scaling([sigs[0]], [(1.0, 2.0, 0.0)])
    assert np.isinf(sc0[0])


def test_scaling_helper_accepts_triples_arrays_and_meta_dicts():
    from sloika_amd import batch
    reads = [np.arange(10, dtype=np.int16), np.arange(7, dtype=np.int16)]
    trip = [(33.0, 1373.41, 8192.0), (-12.5, 1516.72, 2048.0)]
    want = batch.adc_scaling(reads, trip)
    arr = np.asarray(trip)
    meta = [{"digitisation": d, "offset": o, "range": r, "sampling_rate": 4000.0} for o, r, d in trip]
    for form in (arr, meta, tuple(trip), [list(t) for t in trip]):
        got = batch.adc_scaling(reads, form)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # chunks: one [n, L] int16 matrix, one scaling per row
    got = batch.adc_scaling(np.zeros((2, 40), dtype=np.int16), trip)
    assert np.array_equal(got[1], want[1])


def test_scaling_helper_refuses_mismatches():
    from sloika_amd import batch
    reads = [np.arange(10, dtype=np.int16), np.arange(7, dtype=np.int16)]
    trip = [(33.0, 1373.41, 8192.0), (-12.5, 1516.72, 2048.0)]
    with pytest.raises(ValueError):
        batch.adc_scaling(reads, trip[:1])                                   # count
    with pytest.raises(ValueError):
        batch.adc_scaling(reads[:1], trip)
    with pytest.raises(ValueError):
        batch.adc_scaling(reads, np.ones((2, 4)))                            # not [n, 3]
    with pytest.raises(ValueError):
        batch.adc_scaling(reads, [(1.0, 2.0), (1.0, 2.0)])
    with pytest.raises(TypeError):
        batch.adc_scaling([reads[0].astype(np.float32), reads[1]], trip)     # dtype
    with pytest.raises(TypeError):
        batch.adc_scaling([reads[0].astype(np.int32), reads[1]], trip)
    with pytest.raises(TypeError):
        batch.adc_scaling([reads[0].reshape(2, 5), reads[1]], trip)          # rank
    with pytest.raises(TypeError):
        batch.adc_scaling([list(range(10)), reads[1]], trip)                 # not an array
    with pytest.raises(TypeError):
        batch.adc_scaling(np.zeros((2, 40), dtype=np.float32), trip)         # float chunks
    with pytest.raises(TypeError):
        batch.adc_scaling(np.zeros(40, dtype=np.int16), trip)                # chunks must be [n, L]


@pytest.mark.skipif(not have_ref, reason="reference checkout not present (GPU box)")
def test_fast5_scaling_is_the_int16_twin_of_get_read():
    from sloika_amd import batch, fast5
    for n in range(1, 9):
        f = fast5.Fast5(os.path.join(REF_READS, "read%d.fast5" % n))
        off, rng, dig = f.scaling()
        assert all(type(v) is float for v in (off, rng, dig))
        m = f.channel_meta
        assert (off, rng, dig) == (float(m["offset"]), float(m["range"]), float(m["digitisation"]))
        adc = f.get_read(scale=False)
        o, s = batch.adc_scaling([adc], [f.scaling()])
        twin = (adc.astype(np.float64) + o[0]) * s[0]
        assert np.array_equal(twin.view(np.uint64), f.get_read().view(np.uint64))
        o2, s2 = batch.adc_scaling([adc], [f.channel_meta])
        assert o2[0] == o[0] and s2[0] == s[0]
