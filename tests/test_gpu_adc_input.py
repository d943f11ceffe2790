"""int16 ADC input on the device: slk_adc_to_pa_i16 against numpy's float64 scaling (fast5 get_read, sloika/basecall.py:105) bit for
bit, and every `scaling=` entry point of pipeline.Basecaller against the same call on the picoamperes."""
import os

import numpy as np
import pytest

from tests.gpu_util import dev, need_gpu, stream

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = np.uint32(0x7fc0dead)


def _expect(adc, off, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((adc.astype(np.float64) + off) * scale).astype(np.float32)


def _run_kernel(torch, src16, start, lens, strides, off, scale, total, src_shift=0, with_flags=True):
    """slk_adc_to_pa_i16 through the C ABI; src_shift moves the input base by that many samples (the input and the output then sit at
    offsets that differ mod 4: the scalar path).  -> (output as uint32 bits, flags)."""
    from sloika_amd import _lib
    n = len(lens)
    s = dev(np.concatenate([np.zeros(src_shift, dtype=np.int16), src16]))
    out = torch.from_numpy(np.full(total, CANARY, dtype=np.uint32).view(np.float32)).cuda()
    flags = torch.zeros((n,), dtype=torch.int32, device="cuda")
    st, ln, sd = dev(np.asarray(start, np.int64)), dev(np.asarray(lens, np.int32)), dev(np.asarray(strides, np.int32))
    od, sc = dev(np.asarray(off, np.float64)), dev(np.asarray(scale, np.float64))
    rc = _lib.lib().slk_adc_to_pa_i16(s.data_ptr() + 2 * src_shift, st.data_ptr(), ln.data_ptr(), sd.data_ptr(), od.data_ptr(),
                                      sc.data_ptr(), n, int(max(strides)), out.data_ptr(), flags.data_ptr() if with_flags else None,
                                      stream())
    _lib.check(rc, "adc_to_pa")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), flags.cpu().numpy()


def _check_reads(got, src16, start, lens, strides, off, scale, total):
    covered = np.zeros(total, dtype=bool)
    for r in range(len(lens)):
        a, n, s = start[r], lens[r], strides[r]
        want = _expect(src16[a:a + n], off[r], scale[r])
        g = got[a:a + n]
        nan = np.isnan(want)
        assert np.array_equal(g[~nan], want[~nan].view(np.uint32)), r
        assert np.isnan(g[nan].view(np.float32)).all(), r
        assert (got[a + n:a + s] == 0).all(), r                    # the pad is +0.0 (bits 0), not (0 + offset) * scale
        covered[a:a + s] = True
    assert (got[~covered] == CANARY).all()                         # nothing outside [start, start + stride) written


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("src_shift", [0, 1])
def test_kernel_bits_pad_and_canaries(aligned, src_shift):
    torch = need_gpu()
    rs = np.random.RandomState(5 + aligned + 2 * src_shift)
    g = np.load(os.path.join(GOLDEN, "reads.npz"))
    nread = 40
    lens = rs.randint(1, 3000, size=nread)
    lens[:6] = [1, 2, 3, 4, 5, 4001]
    strides = -(-lens // 100) * 100 if aligned else lens + rs.randint(0, 9, size=nread)
    strides[7] = lens[7] = 0                                       # an empty read
    gaps = rs.randint(1, 3, size=nread) * 100 if aligned else rs.randint(1, 13, size=nread) * 2 + 1
    start = np.concatenate([[gaps[0]], np.cumsum(strides + gaps)[:-1] + gaps[0]]).astype(np.int64)
    total = int(start[-1] + strides[-1] + 16)
    src = rs.randint(-32768, 32768, size=total).astype(np.int16)
    src[start[5]:start[5] + 3] = [-32768, 32767, 0]
    dig = rs.choice([8192.0, 2048.0], size=nread)
    rng = rs.uniform(200.0, 3000.0, size=nread)
    off = rs.uniform(-400.0, 400.0, size=nread)
    for k, n in enumerate((3, 5)):                                 # the real channels: meta = [digitisation, offset, range, rate]
        dig[10 + k], off[10 + k], rng[10 + k] = g["meta_%d" % n][:3]
    scale = rng / dig
    got, flags = _run_kernel(torch, src, start, lens, strides, off, scale, total, src_shift)
    _check_reads(got, src, start, lens, strides, off, scale, total)
    assert (flags == 0).all()


def test_kernel_flags_reads_that_are_not_finite():
    torch = need_gpu()
    rs = np.random.RandomState(8)
    lens = np.array([500, 333, 1000, 7, 64, 900], dtype=np.int64)
    strides = -(-lens // 100) * 100
    start = np.concatenate([[0], np.cumsum(strides)[:-1]]).astype(np.int64)
    total = int(strides.sum())
    src = rs.randint(-2000, 2000, size=total).astype(np.int16)
    off = np.array([10.0, np.nan, -3.0, 1.0, 5.0, 0.0])
    rng = np.array([1400.0, 1400.0, 1400.0, 1400.0, 1e30, 1400.0])
    dig = np.array([8192.0, 8192.0, 0.0, 2048.0, 1e-30, 8192.0])
    with np.errstate(divide="ignore"):
        scale = rng / dig                                          # read 2: inf; read 4: 1e60 -> overflows float32
    src[start[5]:start[5] + lens[5]] = 0                           # finite, all zero
    got, flags = _run_kernel(torch, src, start, lens, strides, off, scale, total)
    _check_reads(got, src, start, lens, strides, off, scale, total)
    assert flags.tolist() == [0, 1, 1, 0, 1, 0]
    got2, flags2 = _run_kernel(torch, src, start, lens, strides, off, scale, total, with_flags=False)     # flags are nullable
    assert np.array_equal(got, got2) and (flags2 == 0).all()


def test_kernel_more_reads_than_the_grid_holds():
    torch = need_gpu()
    rs = np.random.RandomState(2)
    nread = 70001
    lens = rs.randint(0, 6, size=nread)
    strides = lens + rs.randint(0, 3, size=nread)
    start = np.concatenate([[0], np.cumsum(strides)[:-1]]).astype(np.int64)
    total = int(strides.sum()) + 8
    src = rs.randint(-32768, 32768, size=total).astype(np.int16)
    off = rs.uniform(-100.0, 100.0, size=nread)
    off[nread - 3] = np.nan                                        # a read past the first 65535
    scale = rs.uniform(100.0, 2000.0, size=nread) / 8192.0
    got, flags = _run_kernel(torch, src, start, lens, strides, off, scale, total)
    _check_reads(got, src, start, lens, strides, off, scale, total)
    assert np.flatnonzero(flags).tolist() == ([nread - 3] if lens[nread - 3] else [])


# ---- end to end: the int16 flows against the picoamperes ----------------------------------------------------------------------------
def _pretrained():
    from sloika_amd import models
    return models.from_weights_npz(os.path.join(GOLDEN, "pretrained_weights.npz"))


def _rgrgr():
    from sloika_amd import models
    return models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=17))


@pytest.mark.parametrize("fraction", [0.0, 0.3])
def test_call_reads_real_reads_equal_picoampere_path(fraction):
    need_gpu()
    from sloika_amd import pipeline
    g = np.load(os.path.join(GOLDEN, "reads.npz"))
    adc, trip, pa = [], [], []
    for n in (3, 5):
        dig, off, rng, _rate = (float(v) for v in g["meta_%d" % n])
        adc.append(g["adc_%d" % n])
        trip.append((off, rng, dig))
        pa.append((g["adc_%d" % n].astype(np.float64) + off) * (rng / dig))          # fast5.Fast5.get_read(raw=True)
    adc.append(g["adc_5"][3000:9123])                                                   # a third read, cut from the other
    trip.append(trip[1])
    pa.append(pa[1][3000:9123])
    bc = pipeline.Basecaller(_pretrained(), kmer_len=5, min_prob=1e-5, skip=5.0)
    s0, p0, l0, n0 = bc.call_reads(pa, trim=(200, 10), open_pore_fraction=fraction)
    s1, p1, l1, n1 = bc.call_reads(adc, trim=(200, 10), open_pore_fraction=fraction, scaling=trip)
    assert n1 == n0
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s0.cpu().numpy().view(np.uint32))
    assert np.array_equal(l1.cpu().numpy(), l0.cpu().numpy()) and np.array_equal(p1.cpu().numpy(), p0.cpu().numpy())
    # the same ValueErrors as the picoampere call
    with pytest.raises(ValueError, match="shorter than one window"):
        bc.call_reads([adc[0], adc[0][:99]], scaling=trip[:2])
    with pytest.raises(ValueError, match="empty read after trimming"):
        bc.call_reads([adc[0], adc[0][:300]], trim=(200, 100), scaling=trip[:2])
    with pytest.raises(ValueError, match="empty read after trimming"):
        bc.call_reads([pa[0], pa[0][:300]], trim=(200, 100))
    # more taken off the end than the read holds: nothing left (the reference's x[a:-b]), not samples from the wrong end
    with pytest.raises(ValueError, match="empty read after trimming"):
        bc.call_reads([adc[0], adc[0][:300]], trim=(0, 400), scaling=trip[:2])
    with pytest.raises(ValueError, match="empty read after trimming"):
        bc.call_reads([pa[0], pa[0][:300]], trim=(0, 400))
    nan_read = pa[0].copy()
    nan_read[1234] = np.nan
    with pytest.raises(ValueError, match="read 1 holds samples that are not finite"):
        bc.call_reads([pa[0], nan_read])
    with pytest.raises(TypeError):
        bc.call_reads([pa[0]], scaling=trip[:1])                                        # float64 samples with a scaling


def _synthetic_adc_reads(n, seed, lo=1500, hi=5000):
    from sloika_amd import pipeline
    rs = np.random.RandomState(seed)
    base = pipeline.synthetic_chunks(4, chunk_len=hi + 600, seed=seed)
    trip = np.stack([rs.uniform(-30.0, 40.0, n), rs.uniform(1200.0, 1600.0, n), np.full(n, 8192.0)], axis=1)
    trip[::3, 2] = 2048.0
    adc = []
    for i, ln in enumerate(rs.randint(lo, hi, size=n)):
        pa = base[i % 4][rs.randint(0, 500):][:ln].astype(np.float64)
        adc.append(np.clip(np.rint(pa / (trip[i, 1] / trip[i, 2]) - trip[i, 0]), -32768, 32767).astype(np.int16))
    return adc, trip


def _pa(adc, trip):
    return [(a.astype(np.float64) + t[0]) * (t[1] / t[2]) for a, t in zip(adc, trip)]


@pytest.mark.parametrize("stream_buckets", [True, False])
def test_call_reads_bucketed_equals_float64_input(stream_buckets, capsys):
    need_gpu()
    from sloika_amd import pipeline
    adc, trip = _synthetic_adc_reads(13, seed=21)
    trip[4, 0] = np.nan                                            # every sample not finite
    adc[9] = adc[9][:60]                                           # shorter than one window
    pa = _pa(adc, trip)
    net = _rgrgr()
    kw = dict(max_batch=4, max_waste=0.2, in_flight=2, kmer_len=5, skip=0.0, trim=(37, 112), stream_buckets=stream_buckets)
    capsys.readouterr()
    s0, p0, n0, st0 = pipeline.Basecaller.call_reads_bucketed(net, pa, **kw)
    err0 = capsys.readouterr().err
    s1, p1, n1, st1 = pipeline.Basecaller.call_reads_bucketed(net, adc, scaling=trip, **kw)
    err1 = capsys.readouterr().err
    assert bool(st1.get("streamed")) == stream_buckets and bool(st0.get("streamed")) == stream_buckets
    assert st1["failed"] == st0["failed"] == [4, 9]
    assert sorted(err1.splitlines()) == sorted(err0.splitlines()) and "Failure calling read 4: samples that are not finite" in err1
    assert list(n1) == list(n0) and n1[4] == n1[9] == 0
    assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
    assert all((a is None and b is None) or a.tolist() == b.tolist() for a, b in zip(p1, p0))
    # the other reads are unaffected by the two that fail
    keep = [i for i in range(len(adc)) if i not in (4, 9)]
    s2, p2, n2, _ = pipeline.Basecaller.call_reads_bucketed(net, [adc[i] for i in keep], scaling=trip[keep], **kw)
    assert [n1[i] for i in keep] == list(n2)
    assert all(p1[i].tolist() == p2[j].tolist() and float(s1[i]) == float(s2[j]) for j, i in enumerate(keep))
    # prepare_read_batches / run_read_batches: the same
    batches, ns = pipeline.Basecaller.prepare_read_batches(net, adc, trim=(37, 112), max_batch=4, scaling=trip, kmer_len=5, skip=0.0)
    s3, p3 = pipeline.Basecaller.run_read_batches(net, batches, len(ns), kmer_len=5, skip=0.0)
    assert list(ns) == list(n0) and np.array_equal(s3.view(np.uint32), s0.view(np.uint32))


def _chunk_case(nrow=6, length=2000, seed=3):
    from sloika_amd import pipeline
    rs = np.random.RandomState(seed)
    trip = np.stack([rs.uniform(-30.0, 40.0, nrow), rs.uniform(1200.0, 1600.0, nrow), rs.choice([8192.0, 2048.0], nrow)], axis=1)
    pa = pipeline.synthetic_chunks(nrow, chunk_len=length, seed=seed).astype(np.float64)
    adc = np.clip(np.rint(pa / (trip[:, 1:2] / trip[:, 2:3]) - trip[:, 0:1]), -32768, 32767).astype(np.int16)
    pa32 = ((adc.astype(np.float64) + trip[:, 0:1]) * (trip[:, 1:2] / trip[:, 2:3])).astype(np.float32)
    return adc, trip, pa32


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def test_call_chunks_int16_host_and_device_equal_picoampere_chunks():
    torch = need_gpu()
    from sloika_amd import pipeline
    adc, trip, pa32 = _chunk_case()
    net = _rgrgr()
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    want = [t.cpu().numpy() for t in bc.call_chunks(dev(pa32))]
    for x in (adc, dev(adc), torch.from_numpy(adc)):
        assert _same([t.cpu().numpy() for t in bc.call_chunks(x, scaling=trip)], want)
    meta = [{"offset": o, "range": r, "digitisation": d} for o, r, d in trip]
    assert _same([t.cpu().numpy() for t in bc.call_chunks(adc, scaling=meta)], want)
    # borrow=True: the int16 upload and the picoamperes come out of the arena too -- a warm call allocates nothing
    bb = pipeline.Basecaller(net, kmer_len=5, skip=0.0, borrow=True)
    for x in (adc, dev(adc), adc, dev(adc)):                       # (host input takes one buffer more: the int16 upload)
        assert _same([t.cpu().numpy() for t in bb.call_chunks(x, scaling=trip)], want)
    torch.cuda.synchronize()
    grown = bb._arena.grown
    for x in (adc, dev(adc)):
        assert _same([t.cpu().numpy() for t in bb.call_chunks(x, scaling=trip)], want)
    assert bb._arena.grown == grown
    with pytest.raises(TypeError):
        bc.call_chunks(pa32, scaling=trip)
    with pytest.raises(ValueError):
        bc.call_chunks(adc, scaling=trip[:3])


@pytest.mark.parametrize("nfl", [1, 4])
def test_call_batches_mixes_int16_and_float_batches(nfl):
    need_gpu()
    from sloika_amd import pipeline
    net = _rgrgr()
    cases = [_chunk_case(nrow=5, length=1600, seed=s) for s in range(4)]
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    want = [[t.cpu().numpy() for t in bc.call_chunks(dev(pa32))] for _, _, pa32 in cases]
    feed = [(cases[0][0], cases[0][1]), cases[1][2], (dev(cases[2][0]), cases[2][1]), dev(cases[3][2]),
            (dev(cases[1][0]), cases[1][1]), (cases[3][0], cases[3][1])]
    order = [0, 1, 2, 3, 1, 3]
    got = list(pipeline.Basecaller.call_batches(net, feed, in_flight=nfl, kmer_len=5, skip=0.0))
    assert len(got) == len(feed)
    for res, k in zip(got, order):
        B = res[0].shape[0]
        sc, pa, le = want[k]
        assert np.array_equal(res[0].view(np.uint32), sc.view(np.uint32)) and np.array_equal(res[2], le)
        assert np.array_equal(res[1], pa[:B, :res[1].shape[1]])


def test_int16_without_scaling_is_still_the_unscaled_cast():
    """scaling=None is today's behaviour whatever the dtype: int16 chunks are cast to float32 as they are (no scaling)."""
    need_gpu()
    from sloika_amd import pipeline
    adc, _, _ = _chunk_case(nrow=4, length=1600, seed=9)
    bc = pipeline.Basecaller(_rgrgr(), kmer_len=5, skip=0.0)
    want = [t.cpu().numpy() for t in bc.call_chunks(dev(adc.astype(np.float32)))]
    assert _same([t.cpu().numpy() for t in bc.call_chunks(adc)], want)
    assert _same([t.cpu().numpy() for t in bc.call_chunks(dev(adc))], want)
