"""The lattice marginals with checkpointed forward rows (slk_viterbi_marginals_ckpt_f32, decode.viterbi_marginals_batch(checkpoint=),
pipeline.Basecaller.call_reads_bucketed_qual / fastq_bucketed; design/lattice_marginals.md 8).

The yardstick is the stored-row kernel, slk_viterbi_marginals_f32, which tests/test_gpu_lattice_marginals.py pins to the np.longdouble
oracle: every output of the checkpointed kernel has to carry that kernel's bits, for every number of rows per checkpoint.  Nothing
here has a tolerance."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev, stream
from tests.test_gpu_lattice_marginals import (CASES, SENT_D, SENT_F, SENT_I, case_post, make_post, run, same, untouched,
                                              small_model)  # noqa: F401 (small_model: a fixture)

pytestmark = pytest.mark.gpu

KEYS = ("score", "path", "len", "move_row", "conf", "logz", "gamma")
EVERY = (1, 2, 3, 7, 8, 0)


def run_ckpt(post, nbase, klen, skip, mp, every, lens=None, gamma=True, mode=None, ws_short=0):
    """slk_viterbi_marginals_ckpt_f32 on a host posterior [T, B, S] -> (rc, dict of host arrays), as test_gpu_lattice_marginals.run."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, S = post.shape
    N = S - 1
    pd = dev(post)
    need = int(L.slk_viterbi_marginals_ckpt_workspace_bytes(T, B, nbase, klen, max(every, 0)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    out = {"score": dev(np.full(B, SENT_F)), "path": dev(np.full((B, T), SENT_I)), "len": dev(np.full(B, SENT_I)),
           "move_row": dev(np.full((B, T), SENT_I)), "conf": dev(np.full((B, T), SENT_D)), "logz": dev(np.full(B, SENT_D))}
    if gamma:
        out["gamma"] = dev(np.full((T, B, max(N, 1)), SENT_F))
    ld = None if lens is None else dev(np.asarray(lens, dtype=np.int32))
    rc = L.slk_viterbi_marginals_ckpt_f32(pd.data_ptr(), T, B, nbase, klen, float(skip), _lib.POST_RAW if mode is None else mode,
                                          float(mp), None if ld is None else ld.data_ptr(), int(every), ws.data_ptr(),
                                          max(need - ws_short, 0), out["score"].data_ptr(), out["path"].data_ptr(),
                                          out["len"].data_ptr(), out["move_row"].data_ptr(), out["conf"].data_ptr(),
                                          out["logz"].data_ptr(), out["gamma"].data_ptr() if gamma else None, stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


_STORED = {}


def stored(name):
    """The stored-row kernel's outputs for a case of CASES, computed once."""
    if name not in _STORED:
        nbase, klen, T, B, skip, mp, lens, _ = CASES[name]
        post = case_post(name)
        rc, want = run(post, nbase, klen, skip, mp, lens)
        assert rc == 0, name
        _STORED[name] = (post, want)
    return _STORED[name]


# ---- 1: the bits of the stored-row kernel ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_stored_row_kernel(name):
    """All seven outputs, with gamma and the case's ragged lengths, for 1, 2, 3, 7 and 8 rows per checkpoint and the launcher's choice."""
    nbase, klen, T, B, skip, mp, lens, _ = CASES[name]
    post, want = stored(name)
    for every in EVERY:
        rc, got = run_ckpt(post, nbase, klen, skip, mp, every, lens)
        assert rc == 0, (name, every)
        for key in KEYS:
            assert same(got[key], want[key]), (name, every, key)


@pytest.mark.parametrize("T", [16, 24, 25])
def test_last_segment_full_and_of_one_row(T):
    """8 rows per checkpoint at N = 64: T = 16 and 24 end on a full segment, T = 25 has a last segment of one row; chunks of a batch
    end at 1, 8, 9 and T rows."""
    post = make_post(4100 + T, T, 4, 65, True)
    lens = [1, 8, 9, T]
    rc, want = run(post, 4, 3, 5.0, 1e-5, lens)
    rc2, got = run_ckpt(post, 4, 3, 5.0, 1e-5, 8, lens)
    assert rc == 0 and rc2 == 0
    for key in KEYS:
        assert same(got[key], want[key]), key


def test_long_chunk_at_the_default():
    """5000 sharp rows of 64 states at the launcher's own rows per checkpoint (64 for N = 64): 79 segments, the last of 8 rows."""
    post = make_post(4200, 5000, 1, 65, True)
    rc, want = run(post, 4, 3, 0.0, 1e-5)
    rc2, got = run_ckpt(post, 4, 3, 0.0, 1e-5, 0)
    assert rc == 0 and rc2 == 0
    assert want["logz"][0] < 2.0 * np.log(np.finfo(np.float64).tiny)    # an unscaled product would have underflowed long before
    for key in KEYS:
        assert same(got[key], want[key]), key


# ---- 2: a chunk's bits depend on the chunk alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n64_t17_b5", "n125_t17_b5", "n1024_t17_b5"])
def test_same_bits_alone_in_a_batch_and_without_gamma(name):
    """test_gpu_lattice_marginals' property test at 3 rows per checkpoint."""
    K = 3
    nbase, klen, T, B, skip, mp, lens, _ = CASES[name]
    post, want = stored(name)
    rc, got = run_ckpt(post, nbase, klen, skip, mp, K, lens)
    assert rc == 0 and all(same(got[key], want[key]) for key in KEYS)
    rc, bare = run_ckpt(post, nbase, klen, skip, mp, K, lens, gamma=False)
    assert rc == 0
    for key in ("score", "path", "len", "move_row", "conf", "logz"):
        assert same(bare[key], got[key]), key
    for b in (0, B - 1, 2):
        n = T if lens is None else lens[b]
        rc, one = run_ckpt(np.ascontiguousarray(post[:n, b:b + 1]), nbase, klen, skip, mp, K, None)
        assert rc == 0
        for key in ("score", "len", "logz"):
            assert same(one[key], got[key][b:b + 1]), (key, b)
        for key in ("path", "move_row", "conf"):
            assert same(one[key][0], got[key][b, :n]), (key, b)
        assert same(one["gamma"][:, 0], got["gamma"][:n, b]), b
        # ... and with its rows given as a length of a longer chunk
        rc, rag = run_ckpt(np.ascontiguousarray(post[:, b:b + 1]), nbase, klen, skip, mp, K, [n])
        assert rc == 0 and same(rag["conf"], got["conf"][b:b + 1]) and same(rag["gamma"][:, 0], got["gamma"][:, b])


# ---- 3: refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    from sloika_amd import _lib
    post = make_post(5, 10, 2, 65, False)
    rc, out = run_ckpt(post, 4, 3, 0.0, 1e-5, -1)
    assert rc == _lib.SLK_ERR_INVALID_ARG and untouched(out)
    big = make_post(6, 4, 1, 1025, False)
    rc, out = run_ckpt(big, 4, 5, 0.0, 1e-5, 16)                   # 9 * 1024 * 16 bytes of segment beside 21568: above 160 KiB
    assert rc == _lib.SLK_ERR_UNSUPPORTED and untouched(out)
    rc, out = run_ckpt(big, 4, 5, 0.0, 1e-5, 15)                   # ... and 15 rows fit
    assert rc == 0 and not untouched(out)
    rc, out = run_ckpt(post, 4, 3, 0.0, 1e-5, 4, ws_short=1)
    assert rc == _lib.SLK_ERR_WORKSPACE and untouched(out)
    for mode in (_lib.POST_LOG, _lib.POST_LN):
        rc, out = run_ckpt(post, 4, 3, 0.0, 1e-5, 4, mode=mode)
        assert rc == _lib.SLK_ERR_UNSUPPORTED and untouched(out)
    for nbase, klen, S in ((4, 6, 4097), (5, 5, 3126)):            # N > 1024
        rc, out = run_ckpt(make_post(5, 4, 2, S, False), nbase, klen, 0.0, 1e-5, 2)
        assert rc == _lib.SLK_ERR_UNSUPPORTED and untouched(out), (nbase, klen)
    rc, out = run_ckpt(post, 4, 3, 0.0, 1e-5, 4)
    assert rc == 0 and not untouched(out)


# ---- 5: decode.viterbi_marginals_batch(checkpoint=) ---------------------------------------------------------------------------------

def test_viterbi_marginals_batch_checkpoint():
    need_gpu()
    from sloika_amd import decode
    nbase, klen, T, B, skip, mp, lens, _ = CASES["n1024_t17_b5"]
    post = dev(case_post("n1024_t17_b5"))
    ragged = [17, 1, 9, 16, 4]
    for lengths in (None, ragged):
        want = [t.cpu().numpy() for t in decode.viterbi_marginals_batch(post, klen, skip_pen=skip, lengths=lengths, gamma=True)]
        for checkpoint in (True, 3):
            got = decode.viterbi_marginals_batch(post, klen, skip_pen=skip, lengths=lengths, gamma=True, checkpoint=checkpoint)
            assert len(got) == 7 and all(same(g.cpu().numpy(), w) for g, w in zip(got, want)), (lengths, checkpoint)
            # two chunks per launch: three launches for the five
            alone = decode.marginals_workspace_bytes(T, 1, nbase, klen, checkpoint)
            assert 2 * alone < decode.marginals_workspace_bytes(T, 3, nbase, klen, checkpoint)
            split = decode.viterbi_marginals_batch(post, klen, skip_pen=skip, lengths=lengths, gamma=True, checkpoint=checkpoint,
                                                   workspace_limit=2 * alone)
            assert all(same(g.cpu().numpy(), w) for g, w in zip(split, want)), (lengths, checkpoint)
            with pytest.raises(ValueError):
                decode.viterbi_marginals_batch(post, klen, checkpoint=checkpoint, workspace_limit=alone - 1)
    for bad in (0, -2, 2.5, False):
        with pytest.raises(ValueError):
            decode.viterbi_marginals_batch(post, klen, checkpoint=bad)


# ---- 6: the bucketed flow --------------------------------------------------------------------------------------------------------------

LENGTHS = (6000, 5100, 4300, 3500, 2800, 2100, 1500)
KW = dict(kmer_len=5, skip=5.0, trim=(50, 20))


@pytest.fixture(scope="module")
def read_set(small_model):
    """Seven synthetic reads of clearly different lengths as int16 ADC samples with their scalings and as the float64 picoamperes
    those scale to, a read of 50 samples and one holding a NaN; per good read what the single-read calls give."""
    from sloika_amd import pipeline
    rs = np.random.RandomState(31)
    base = pipeline.synthetic_chunks(len(LENGTHS), chunk_len=max(LENGTHS), seed=31)
    n = len(LENGTHS) + 2
    trip = np.stack([rs.uniform(-30.0, 40.0, n), rs.uniform(1200.0, 1600.0, n), np.full(n, 8192.0)], axis=1)
    adc = []
    for i in range(n):
        pa = base[i % len(LENGTHS)][:LENGTHS[i] if i < len(LENGTHS) else 3000].astype(np.float64)
        adc.append(np.clip(np.rint(pa / (trip[i, 1] / trip[i, 2]) - trip[i, 0]), -32768, 32767).astype(np.int16))
    adc[7] = adc[7][:50]                                           # shorter than one window
    pa = [(a.astype(np.float64) + t[0]) * (t[1] / t[2]) for a, t in zip(adc, trip)]
    pa[8][1234] = np.nan
    trip_nan = trip.copy()
    trip_nan[8, 0] = np.nan                                        # the int16 twin of the read that is not finite
    names = ["r%d" % i for i in range(n)]
    bc = pipeline.Basecaller(small_model, kmer_len=5, skip=5.0)
    single = []
    for i in range(len(LENGTHS)):
        res = bc.call_reads_qual([pa[i]], trim=KW["trim"])
        k = int(res[2].cpu().numpy()[0])
        single.append({"score": res[0].cpu().numpy()[0], "path": res[1].cpu().numpy()[0, :k], "move_row": res[3].cpu().numpy()[0, :k],
                       "conf": res[4].cpu().numpy()[0, :k], "logz": res[5].cpu().numpy()[0], "nsamp": res[6][0],
                       "fastq": bc.call_fastq([pa[i]], names=[names[i]], trim=KW["trim"])[0]})
    return {"net": small_model, "pa": pa, "adc": adc, "trip": trip_nan, "names": names, "single": single, "bc": bc}


def check_reads(read_set, res):
    scores, paths, rows, confs, logz, nsamp, stats = res
    assert scores.dtype == np.float32 and logz.dtype == np.float64 and len(paths) == len(rows) == len(confs) == 9
    assert stats["failed"] == [7, 8] and stats["reads"] == 9
    for i in (7, 8):
        assert np.isnan(scores[i]) and np.isnan(logz[i]) and paths[i] is None and rows[i] is None and confs[i] is None and nsamp[i] == 0
    for i, one in enumerate(read_set["single"]):
        assert nsamp[i] == one["nsamp"], i
        assert same(scores[i:i + 1], np.array([one["score"]])) and same(logz[i:i + 1], np.array([one["logz"]])), i
        assert same(paths[i], one["path"]) and same(rows[i], one["move_row"]) and same(confs[i], one["conf"]), i


def test_bucketed_qual_equals_the_single_read_calls(read_set, capsys):
    need_gpu()
    from sloika_amd import decode, pipeline
    res = pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], in_flight=2, **KW)
    err = capsys.readouterr().err
    assert "Failure calling read 7" in err and "Failure calling read 8: samples that are not finite" in err
    check_reads(read_set, res)
    stats = res[-1]
    assert stats["rows_per_checkpoint"] == decode.marginals_default_rows(4, 5) == 4 and stats["lanes"] == 2
    assert stats["peak_bucket_bytes"] <= stats["memory_limit"] // 2
    # a number of rows per checkpoint of the caller's
    res3 = pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], in_flight=2, checkpoint=3, **KW)
    check_reads(read_set, res3)
    assert res3[-1]["rows_per_checkpoint"] == 3


def test_bucketed_qual_memory_limit(read_set):
    """With max_waste 0.9 the seven good reads are one bucket by length; a limit that gives each of two lanes room for two reads of
    the longest's length forces at least three.  The same bytes, and the largest bucket within its lane's share."""
    need_gpu()
    from sloika_amd import pipeline
    bc = read_set["bc"]
    nlong = LENGTHS[0] - sum(KW["trim"])
    kw = dict(KW, max_waste=0.9, in_flight=2)
    free = pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], **kw)
    assert free[-1]["batches"] == 1
    check_reads(read_set, free)
    limit = 2 * bc.qual_footprint(nlong, 2)
    assert bc.qual_footprint(nlong, 2) < bc.qual_footprint(nlong, 3)
    res = pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], memory_limit=limit, **kw)
    check_reads(read_set, res)
    stats = res[-1]
    assert stats["batches"] >= 3 and stats["memory_limit"] == limit and stats["lanes"] == 2
    assert 0 < stats["peak_bucket_bytes"] <= limit / 2
    assert stats["peak_bucket_bytes"] == bc.qual_footprint(nlong, 2)
    # a read that outgrows the share on its own is named before anything runs
    with pytest.raises(ValueError, match="read 0"):
        pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], memory_limit=bc.qual_footprint(nlong, 1) - 1,
                                                     **dict(kw, in_flight=1))
    with pytest.raises(ValueError, match="read 0"):
        pipeline.Basecaller.call_reads_bucketed_qual(read_set["net"], read_set["pa"], memory_limit=2 * bc.qual_footprint(nlong, 1) - 2,
                                                     **kw)


def test_fastq_bucketed_equals_call_fastq(read_set):
    need_gpu()
    from sloika_amd import pipeline
    recs = pipeline.Basecaller.fastq_bucketed(read_set["net"], read_set["pa"], names=read_set["names"], in_flight=2, **KW)
    assert len(recs) == 9 and recs[7] is None and recs[8] is None
    for i, one in enumerate(read_set["single"]):
        assert recs[i] == one["fastq"], i
        assert recs[i].startswith("@r%d\n" % i) and recs[i].count("\n") == 4
    # int16 reads with their scalings: the same records as their picoamperes
    adc = pipeline.Basecaller.fastq_bucketed(read_set["net"], read_set["adc"], names=read_set["names"], in_flight=2,
                                             scaling=read_set["trip"], **KW)
    assert adc == recs
    unnamed = pipeline.Basecaller.fastq_bucketed(read_set["net"], read_set["pa"][:2], in_flight=1, **KW)
    assert [r.split("\n")[0] for r in unnamed] == ["@read0", "@read1"]
    assert unnamed[0].split("\n")[1:] == recs[0].split("\n")[1:]


# ---- 7: non-transducer models ----------------------------------------------------------------------------------------------------------

def test_non_transducer_model_is_refused(small_model):
    need_gpu()
    from sloika_amd import pipeline
    reads = [pipeline.synthetic_chunks(1, chunk_len=1500, seed=3)[0]]
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller.call_reads_bucketed_qual(small_model, reads, kmer_len=5, transducer=False)
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller.fastq_bucketed(small_model, reads, kmer_len=5, transducer=False)
