"""GPU parity: median/MAD normalisation at every kernel boundary, at the selection kernel's collected-key limit, with padded
strides, in its ragged whole-read form, and the two helpers of the same read path (slk_pack_reads_f32, slk_reads_nonfinite_f32).

slk_med_mad_normalise_f32 picks one of four kernels by length (csrc/frontend.hip): the LDS bitonic sort for 1..1023 and
4097..32768 samples, med_mad_select_kernel<8> for 1024..2048, <16> for 2049..4096, radix selection above 32768;
slk_med_mad_normalise_ragged_f32 is radix selection at every length.  The contract is numpy's float32 evaluation bit for bit,
so nothing here has a tolerance: results are compared by value with the oracle (tests/test_oracle_signal.py pins it to numpy on
the same inputs), and bit patterns are compared where the library is compared with itself or with what it must not touch.
"""
import numpy as np
import pytest

from tests import normalise_cases as cases
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                      # a quiet NaN no kernel here produces: "nobody wrote this word"


def sentinel(torch, n):
    return torch.full((int(n),), SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    """Device tensor (any 4-byte type) -> its words on the host."""
    return t.contiguous().view(-1).cpu().numpy().view(np.uint32)


def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dv(a):
    """A copy on the device (the shared fixtures are read-only arrays)."""
    return dev(np.array(a))


def oracle_ref(oracle, x):
    with np.errstate(all="ignore"):
        return oracle.med_mad_normalise(x, return_stats=True)


# ------------------------------------------------------------------------------------------------------------------
# a. dispatch boundaries
# ------------------------------------------------------------------------------------------------------------------
#: both sides of every hand-over between kernels (1023|1024, 2048|2049, 4096|4097, 32768|32769), the sort kernel's LDS requests
#: around 64 KiB (8192: 32 KiB; 8193 and 16384: exactly 64 KiB on top of 4 static bytes; 16385..32768: 128 KiB, the request that
#: first raises the kernel's dynamic LDS limit), and the smallest odd and even counts
BOUNDARY_LENGTHS = (1, 2, 3, 4, 5, 1023, 1024, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32767, 32768, 32769)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("n", BOUNDARY_LENGTHS)
def test_dispatch_boundaries_vs_oracle(oracle, n, kind):
    need_gpu()
    from sloika_amd import batch
    x = cases.make(kind, n, 3, seed=n)
    ref, rmed, rmad = oracle_ref(oracle, x)
    out, med, mad = batch.normalise_chunks(x, 'per-chunk', return_stats=True)
    assert np.array_equal(med, rmed) and np.array_equal(mad, rmad)
    assert np.array_equal(out, ref, equal_nan=True)
    net = batch.normalise_chunks(x, 'per-chunk', out_layout='network')
    assert net.shape == (n, 3, 1)
    assert np.array_equal(fbits(net[:, :, 0].T), fbits(out))               # the same kernel through other strides: bit for bit


# ------------------------------------------------------------------------------------------------------------------
# b. the selection kernel's collected-key limit (SEL_CAP = 256)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1500, 1501, 4000, 4001])
@pytest.mark.parametrize("where", cases.WHERE)
@pytest.mark.parametrize("m", [255, 256, 257])
def test_selection_collects_255_256_257_keys(oracle, m, where, n):
    """m samples share the median's upper 16 key bits: one below, exactly at and one above what wave 0 finishes alone; the wanted
    rank on the group's first, middle and last element (with 'last' and an even count the upper neighbour is the smallest key
    outside the group); both register footprints, odd and even counts, ten shuffles."""
    need_gpu()
    from sloika_amd import batch
    x = cases.group(n, m, where, nchunk=10, seed=n + m)
    assert [cases.upper16_count(row) for row in x] == [m] * 10
    ref, rmed, rmad = oracle_ref(oracle, x)
    out, med, mad = batch.normalise_chunks(x, 'per-chunk', return_stats=True)
    assert np.array_equal(med, rmed) and np.array_equal(mad, rmad)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("where", cases.WHERE)
@pytest.mark.parametrize("m", [127, 128, 129])
def test_selection_collects_254_256_258_deviations(oracle, m, where, n):
    """The same limit in the MAD pass: the median is exactly 0 and every constructed magnitude appears twice among |x - med|."""
    need_gpu()
    from sloika_amd import batch
    x = cases.mirrored(n, m, where, nchunk=10, seed=n + m)
    assert np.all(np.median(x, axis=1) == 0)
    assert [cases.upper16_count(np.abs(row)) for row in x] == [2 * m] * 10
    ref, rmed, rmad = oracle_ref(oracle, x)
    out, med, mad = batch.normalise_chunks(x, 'per-chunk', return_stats=True)
    assert np.all(med == 0) and np.array_equal(med, rmed) and np.array_equal(mad, rmad)
    assert np.array_equal(out, ref)


# ------------------------------------------------------------------------------------------------------------------
# c. strides and optional outputs, through the C ABI
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clen", [700, 1500, 4000, 20000, 40000])            # sort, select<8>, select<16>, sort above 64 KiB, radix
def test_padded_strides_and_null_stats(oracle, clen):
    torch = need_gpu()
    from sloika_amd import _lib
    f = _lib.lib().slk_med_mad_normalise_f32
    nchunk, pad = 3, 7
    x = cases.make("rounded", clen, nchunk, seed=clen)
    ref, rmed, rmad = oracle_ref(oracle, x)
    xd = dev(x)
    ocs = clen + pad
    out, med, mad = sentinel(torch, nchunk * ocs), sentinel(torch, nchunk), sentinel(torch, nchunk)
    assert f(xd.data_ptr(), nchunk, clen, out.data_ptr(), ocs, 1, med.data_ptr(), mad.data_ptr(), stream()) == _lib.SLK_OK
    got = bits(out).reshape(nchunk, ocs)
    assert np.all(got[:, clen:] == SENT)                                    # the gaps between chunks are nobody's
    assert np.array_equal(got[:, :clen].view(np.float32), ref)
    assert np.array_equal(med.cpu().numpy(), rmed) and np.array_equal(mad.cpu().numpy(), rmad)
    out2 = sentinel(torch, nchunk * ocs)
    assert f(xd.data_ptr(), nchunk, clen, out2.data_ptr(), ocs, 1, None, None, stream()) == _lib.SLK_OK
    assert np.array_equal(bits(out2), bits(out))
    # sample-major with room behind every time step: element (c, i) at i * (nchunk + 2) + c
    oss = nchunk + 2
    out3 = sentinel(torch, clen * oss)
    assert f(xd.data_ptr(), nchunk, clen, out3.data_ptr(), 1, oss, None, None, stream()) == _lib.SLK_OK
    got3 = bits(out3).reshape(clen, oss)
    assert np.all(got3[:, nchunk:] == SENT)
    assert np.array_equal(got3[:, :nchunk].T, got[:, :clen])


def test_normalise_argument_checks_write_nothing():
    torch = need_gpu()
    from sloika_amd import _lib
    f = _lib.lib().slk_med_mad_normalise_f32
    xd = dev(cases.make("normal", 64, 2, seed=0))
    out, med, mad = sentinel(torch, 256), sentinel(torch, 2), sentinel(torch, 2)
    args = (out.data_ptr(), 64, 1, med.data_ptr(), mad.data_ptr(), stream())
    assert f(xd.data_ptr(), 0, 64, *args) == _lib.SLK_OK
    assert f(xd.data_ptr(), 2, 0, *args) == _lib.SLK_ERR_INVALID_ARG
    assert f(None, 2, 64, *args) == _lib.SLK_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert np.all(bits(out) == SENT) and np.all(bits(med) == SENT) and np.all(bits(mad) == SENT)


# ------------------------------------------------------------------------------------------------------------------
# d. ragged form
# ------------------------------------------------------------------------------------------------------------------
RAGGED_LENS = (1, 2, 3, 64, 1023, 1024, 4097, 33000, 0, 2049)


@pytest.fixture(scope="module")
def ragged_batch():
    """[B, Lmax + 5] float32: read r in the first RAGGED_LENS[r] samples of row r, large finite garbage everywhere else."""
    rs = np.random.RandomState(77)
    B, lmax = len(RAGGED_LENS), max(RAGGED_LENS)
    sig = (rs.uniform(1e29, 1e30, size=(B, lmax + 5)) * rs.choice([-1.0, 1.0], size=(B, lmax + 5))).astype(np.float32)
    for r, n in enumerate(RAGGED_LENS):
        x = (rs.normal(size=n) * 12 + 90).astype(np.float32)
        x[: n // 3] = np.round(x[: n // 3] * 4) / 4                         # duplicates
        sig[r, :n] = x
    sig.setflags(write=False)
    return sig


def run_ragged(torch, sig, lens, layout):
    """-> (words of out as [B, row], words of med, words of mad); row = in_stride + 3 words per read in either layout."""
    from sloika_amd import _lib
    B, in_stride = sig.shape
    row = in_stride + 3
    sd, ld = dv(sig), dev(np.asarray(lens, dtype=np.int32))
    out, med, mad = sentinel(torch, B * row), sentinel(torch, B), sentinel(torch, B)
    ocs, oss = (row, 1) if layout == "chunk" else (1, B)
    rc = _lib.lib().slk_med_mad_normalise_ragged_f32(sd.data_ptr(), B, in_stride, ld.data_ptr(), out.data_ptr(), ocs, oss,
                                                     med.data_ptr(), mad.data_ptr(), stream())
    assert rc == _lib.SLK_OK
    w = bits(out)
    w = w.reshape(B, row) if layout == "chunk" else np.ascontiguousarray(w.reshape(row, B).T)
    return w, bits(med), bits(mad)


@pytest.mark.parametrize("layout", ["chunk", "network"])
def test_ragged_reads_vs_oracle_and_vs_each_read_alone(oracle, ragged_batch, layout):
    torch = need_gpu()
    from sloika_amd import _lib
    sig = ragged_batch
    w, med, mad = run_ragged(torch, sig, RAGGED_LENS, layout)
    alone = _lib.lib().slk_med_mad_normalise_f32
    for r, n in enumerate(RAGGED_LENS):
        assert np.all(w[r, n:] == SENT), r                                  # nothing behind the read is written
        if n == 0:
            assert med[r] == SENT and mad[r] == SENT                        # an empty read leaves its statistics alone too
            continue
        ref, rmed, rmad = oracle_ref(oracle, sig[r:r + 1, :n])
        # (a read of one sample is 0/0 = NaN); the garbage behind the read is not in the statistics
        assert np.array_equal(w[r, :n].view(np.float32), ref[0], equal_nan=True), r
        assert med[r:r + 1].view(np.float32)[0] == rmed[0] and mad[r:r + 1].view(np.float32)[0] == rmad[0], r
        # the header's promise across kernels: the sort, selection and radix kernels on this read alone give the same bits
        o1, m1, d1 = sentinel(torch, n), sentinel(torch, 1), sentinel(torch, 1)
        assert alone(dv(sig[r, :n]).data_ptr(), 1, n, o1.data_ptr(), n, 1, m1.data_ptr(), d1.data_ptr(), stream()) == _lib.SLK_OK
        assert np.array_equal(bits(o1), w[r, :n]), r
        assert bits(m1)[0] == med[r] and bits(d1)[0] == mad[r], r


def test_ragged_reads_in_reversed_order(ragged_batch):
    torch = need_gpu()
    sig = ragged_batch
    w, med, mad = run_ragged(torch, sig, RAGGED_LENS, "chunk")
    wr, medr, madr = run_ragged(torch, np.ascontiguousarray(sig[::-1]), RAGGED_LENS[::-1], "chunk")
    assert np.array_equal(wr[::-1], w) and np.array_equal(medr[::-1], med) and np.array_equal(madr[::-1], mad)


def test_normalise_reads_ragged_is_zero_behind_each_read(ragged_batch):
    torch = need_gpu()
    from sloika_amd import batch
    sig = ragged_batch
    B, lmax = len(RAGGED_LENS), max(RAGGED_LENS)
    w, _, _ = run_ragged(torch, sig, RAGGED_LENS, "chunk")
    padded = dv(sig[:, :lmax])                                             # [B, Lmax], the garbage behind each read still in it
    out = batch.normalise_reads_ragged(padded, dev(np.asarray(RAGGED_LENS, dtype=np.int32)))
    assert tuple(out.shape) == (lmax, B, 1)
    got = bits(out).reshape(lmax, B).T
    for r, n in enumerate(RAGGED_LENS):
        assert np.array_equal(got[r, :n], w[r, :n]), r
        assert np.all(got[r, n:] == 0), r                                   # +0.0


# ------------------------------------------------------------------------------------------------------------------
# e / f. the read path's helpers: reads of one source buffer -> a zero-padded batch; reads that hold a NaN or an infinity
# ------------------------------------------------------------------------------------------------------------------
READ_LENS = (0, 1, 255, 256, 1023, 1024, 1025, 4095, 4096, 4097, 9000)      # both kernels' block edges: 1024 and 4096 samples


@pytest.fixture(scope="module")
def read_set():
    """(src, start, len): the reads lie in `src` in no particular order, some back to back and some with a gap behind them; every
    sample of `src` is finite and non-zero, the largest float and denormals among them."""
    rs = np.random.RandomState(11)
    order = rs.permutation(len(READ_LENS))
    start = np.zeros(len(READ_LENS), dtype=np.int64)
    pos = 5
    for k, b in enumerate(order):
        start[b] = pos
        pos += READ_LENS[b] + (0 if k % 2 else 3)                           # every other read is followed at once by the next
    src = (rs.normal(size=pos + 16) * 12 + 90).astype(np.float32)
    assert np.all(src != 0)
    big = int(np.argmax(READ_LENS))
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    src[start[big] + np.array([0, 255, 256, 4095, 4096, READ_LENS[big] - 1])] = [fmax, -fmax, tiny, -tiny, fmax, tiny]
    src[start[1]] = -fmax                                                   # the one-sample read
    assert np.all(np.isfinite(src)) and tiny > 0
    src.setflags(write=False)
    start.setflags(write=False)
    return src, start, np.asarray(READ_LENS, dtype=np.int32)


@pytest.mark.parametrize("ld", [9000, 9001, 10240])
def test_pack_reads(read_set, ld):
    torch = need_gpu()
    from sloika_amd import _lib
    src, start, lens = read_set
    B = len(lens)
    want = np.zeros((B, ld), dtype=np.float32)
    for b in range(B):
        want[b, :lens[b]] = src[start[b]:start[b] + lens[b]]
    sd, std, ld_ = dv(src), dv(start), dv(lens)
    dst = sentinel(torch, B * ld)
    f = _lib.lib().slk_pack_reads_f32
    assert f(sd.data_ptr(), std.data_ptr(), ld_.data_ptr(), B, dst.data_ptr(), ld, stream()) == _lib.SLK_OK
    assert np.array_equal(bits(dst).reshape(B, ld), fbits(want))            # the sample, or +0.0: no sentinel, no neighbour's sample


def test_pack_reads_argument_checks_write_nothing(read_set):
    torch = need_gpu()
    from sloika_amd import _lib
    src, start, lens = read_set
    sd, std, ld_ = dv(src), dv(start), dv(lens)
    dst = sentinel(torch, len(lens) * 9000)
    f = _lib.lib().slk_pack_reads_f32
    assert f(sd.data_ptr(), std.data_ptr(), ld_.data_ptr(), 0, dst.data_ptr(), 9000, stream()) == _lib.SLK_OK
    assert f(sd.data_ptr(), std.data_ptr(), ld_.data_ptr(), len(lens), dst.data_ptr(), 0, stream()) == _lib.SLK_ERR_INVALID_ARG
    # more reads than a grid has rows: refused before anything is launched (start / len hold 11 entries)
    assert f(sd.data_ptr(), std.data_ptr(), ld_.data_ptr(), 65536, dst.data_ptr(), 9000, stream()) == _lib.SLK_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.all(bits(dst) == SENT)


def nonfinite_flags(torch, src, start, lens, max_len):
    from sloika_amd import _lib
    sd, std, ld_ = dv(src), dv(start), dv(lens)
    flags = torch.full((len(lens),), 4, dtype=torch.int32, device="cuda")
    rc = _lib.lib().slk_reads_nonfinite_f32(sd.data_ptr(), std.data_ptr(), ld_.data_ptr(), len(lens), max_len, flags.data_ptr(),
                                            stream())
    assert rc == _lib.SLK_OK
    return flags.cpu().numpy()


def expected_flags(src, start, lens):
    return np.array([4 | int(not np.all(np.isfinite(src[s:s + n]))) for s, n in zip(start, lens)], dtype=np.int32)


@pytest.mark.parametrize("max_len", [9000, 10001, 12288])
def test_reads_nonfinite(read_set, max_len):
    """flags[r] |= 1 for exactly the reads that own a NaN or an infinity: at both ends of a read, on both sides of the kernel's 256-
    and 4096-sample strides, and one sample behind a read -- which belongs to the next read in the buffer or to nobody."""
    torch = need_gpu()
    src, start, lens = read_set
    assert np.array_equal(nonfinite_flags(torch, src, start, lens, max_len), np.full(len(lens), 4))     # largest float, denormals
    big, mid = int(np.argmax(lens)), list(lens).index(4097)
    owned_behind = [b for b in range(len(lens)) if np.any(start == start[b] + lens[b]) and lens[b] > 0]
    free_behind = [b for b in range(len(lens)) if not np.any((start <= start[b] + lens[b]) & (start[b] + lens[b] < start + lens))]
    assert owned_behind and free_behind and big in owned_behind + free_behind
    spots = [(big, i) for i in (0, 255, 256, 4095, 4096, int(lens[big]) - 1, int(lens[big]))]
    spots += [(mid, i) for i in (4095, 4096, 4097)]
    spots += [(owned_behind[0], int(lens[owned_behind[0]])), (free_behind[0], int(lens[free_behind[0]]))]
    spots += [(list(lens).index(1), 0), (list(lens).index(0), 0)]
    for bad in (np.nan, np.inf, -np.inf):
        for b, i in spots:
            s = src.copy()
            s[start[b] + i] = bad
            want = expected_flags(s, start, lens)
            assert np.count_nonzero(want == 5) <= 1                         # reads do not overlap: one owner at the most
            if i < lens[b]:
                assert want[b] == 5
            got = nonfinite_flags(torch, s, start, lens, max_len)
            assert np.array_equal(got, want), (bad, b, i)
