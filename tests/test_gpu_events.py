"""The event front end on the GPU: slk_event_features_f32 through the C ABI, and the host interface built on it (features.from_events,
maths.studentise, batch.chunkify / chunkify_many, basecall.events_read_worker, pipeline.Basecaller.call_events), against the outputs
of the reference's own functions stored in tests/golden/events.npz (tests/golden/make_event_goldens.py).

The feature tolerance is measured, not chosen: the reference evaluates in float32, the kernel accumulates in float64 and rounds once;
both are measured against a float64 evaluation of the same formulas (tests/golden/event_cases.py: features64 / studentise64).
e_ref, the reference's largest absolute difference from it over the fixture, is stored in the fixture; e_dev, the device's, is
measured here and must not exceed e_ref plus one float32 ulp of the largest studentised magnitude in the fixture; the comparison
device-vs-fixture gets e_ref + e_dev.  Measured on an MI355X: e_ref = 1.022e-04 (the 10 750-event table: float32 column sums),
e_dev = 2.37e-07, one ulp of the largest magnitude (8.46) = 9.5e-07.
"""
import os
import sys

import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import event_cases as ec  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "events.npz")))


@pytest.fixture(scope="module")
def tables():
    return {name: ec.table(ec.columns(name)) for name in ec.CASES}


def kernel(cols, segs, out_shape, ld_out, normalise=1, nanonet=0, fill=None):
    """slk_event_features_f32 through the C ABI.  cols: [3, N] host array; segs: (start, len, keep, out_row) host sequences.
    -> the float32 output as a host array (filled with `fill` first)."""
    torch = need_gpu()
    from sloika_amd import _lib
    c = dev(np.ascontiguousarray(cols))
    s = dev(np.ascontiguousarray(np.asarray(segs, dtype=np.int64)))
    out = torch.full(out_shape, np.nan if fill is None else fill, dtype=torch.float32, device="cuda")
    rc = _lib.lib().slk_event_features_f32(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), int(cols.dtype == np.float64),
                                           s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), s.shape[1], normalise, nanonet,
                                           out.data_ptr(), s[3].data_ptr(), ld_out, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def whole(name, tables, normalise, nanonet, tag=""):
    from sloika_amd import features
    ev = tables[name]
    n = len(ev)
    return kernel(features.event_columns(ev, tag), ([0], [n], [n], [0]), (n, 4), 4, normalise, nanonet)


def per_chunk(name, tables, cl):
    from sloika_amd import batch, features
    ev = tables[name]
    start, length, keep, row, normalise = batch.event_segments(len(ev), cl, "per-chunk")
    ml = len(ev) // cl
    return kernel(features.event_columns(ev, ""), (start, length, keep, row), (ml, cl, 4), 4, int(normalise))


def exact_zero_columns(f64_raw):
    """Columns whose deviation is exactly 0 (every value the same): both sides give x - m there."""
    return np.ptp(f64_raw, axis=0) == 0


def test_kernel_against_the_fixture(gold, tables):
    """Test 1: every studentised output of the fixture.  Prints the measured figures before it asserts."""
    need_gpu()
    e_ref, max_abs = float(gold["e_ref"]), float(gold["max_abs"])
    ulp = float(np.spacing(np.float32(max_abs)))
    pairs = []                                                  # (what, device float32, fixture float32, float64 yardstick)
    for name in ec.CASES:
        ev = tables[name]
        for normalise in (0, 1):
            for nanonet in (0, 1):
                key = "%s_fe_n%d_k%d" % (name, normalise, nanonet)
                if key not in gold:
                    continue
                got = whole(name, tables, normalise, nanonet)
                f64 = ec.features64(ev, "", bool(normalise), bool(nanonet))
                if not normalise:
                    # the stored values themselves: equal, bit for bit (the nanonet column is compared below)
                    ncol = 3 if nanonet else 4
                    assert np.array_equal(got[:, :ncol], gold[key][:, :ncol]), key
                    if nanonet:
                        pairs.append((key, got[:, 3], gold[key][:, 3], f64[:, 3]))
                    continue
                flat = exact_zero_columns(ec.features64(ev, "", False, False))
                if nanonet:
                    flat[3] = False
                assert np.array_equal(got[:, flat], gold[key][:, flat]), key + ": columns without deviation"
                pairs.append((key, got, gold[key], f64))
        if name + "_fe_scaled" in gold:
            pairs.append((name + "_fe_scaled", whole(name, tables, 1, 0, "scaled_"), gold[name + "_fe_scaled"],
                          ec.features64(ev, "scaled_", True, False)))
        for cl in ec.CHUNK_LENS:
            key = "%s_chunks_%d" % (name, cl)
            if key in gold:
                pairs.append((key, per_chunk(name, tables, cl), gold[key], ec.chunk_features64(ev, "", cl)))
    e_dev = e_ref_here = 0.0
    for key, got, ref, f64 in pairs:
        assert got.shape == ref.shape and got.dtype == np.float32, key
        assert np.array_equal(np.isnan(got), np.isnan(ref)), key     # (one event, nanonet: 0 / 0 on both sides)
        ok = np.isfinite(f64) & np.isfinite(ref)
        if ok.any():
            e_dev = max(e_dev, float(np.abs(got.astype(np.float64) - f64)[ok].max()))
            e_ref_here = max(e_ref_here, float(np.abs(ref.astype(np.float64) - f64)[ok].max()))
    print("e_ref (fixture) %.4e, e_ref over what is compared here %.4e, e_dev %.4e, ulp(%.4f) %.4e"
          % (e_ref, e_ref_here, e_dev, max_abs, ulp))
    assert e_ref_here <= e_ref
    assert e_dev <= e_ref + ulp, (e_dev, e_ref, ulp)
    for key, got, ref, f64 in pairs:
        ok = np.isfinite(ref)
        worst = float(np.abs(got.astype(np.float64) - ref.astype(np.float64))[ok].max()) if ok.any() else 0.0
        assert worst <= e_ref + e_dev, (key, worst)


def check_features(got, ref, bound, what):
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) <= bound, what


def test_host_functions_against_the_fixture(gold, tables):
    """features.from_events and maths.studentise (numpy in, numpy out; device in, device out)."""
    torch = need_gpu()
    from sloika_amd import features, maths
    bound = 2.0 * float(gold["e_ref"]) + float(np.spacing(np.float32(gold["max_abs"])))      # e_ref + (e_dev <= e_ref + ulp)
    for name in ("n2", "n7", "n401", "n2000"):
        ev = tables[name]
        got = features.from_events(ev)
        assert isinstance(got, np.ndarray) and got.flags["C_CONTIGUOUS"]
        check_features(got, gold[name + "_fe_scaled"], bound, name)
        on_dev = features.from_events(ev, tag="", normalise=True, nanonet=True, device=True)
        assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda
        check_features(on_dev.cpu().numpy(), gold[name + "_fe_n1_k1"], bound, name)
        cols = {k: np.asarray(ev[k]) for k in ("mean", "stdv", "length")}                     # a dict of columns
        assert np.array_equal(features.from_events(cols, tag="", normalise=False), gold[name + "_fe_n0_k0"])
    x = ec.studentise_input()
    for key, axis in (("axis0", 0), ("axis1", 1), ("all", None)):
        check_features(maths.studentise(x, axis=axis), gold["studentise_" + key], bound, key)
        y = maths.studentise(dev(x), axis=axis)
        assert isinstance(y, torch.Tensor) and y.is_cuda
        check_features(y.cpu().numpy(), gold["studentise_" + key], bound, key + " on the device")
    # med_mad / mad: numpy's float32 evaluation, bit for bit through the selection kernels, to rounding through the sort
    sig = np.random.RandomState(3).normal(size=(6, 250)).astype(np.float32)

    def ref_med_mad(a, axis):
        med = np.median(a, axis=axis, keepdims=True)
        return med, np.float32(1.4826) * np.median(np.abs(a - med), axis=axis, keepdims=True)
    med, dmad = maths.med_mad(sig, axis=1)
    rmed, rmad = ref_med_mad(sig, 1)
    assert np.array_equal(med, rmed[:, 0]) and np.array_equal(dmad, rmad[:, 0])
    med, dmad = maths.med_mad(sig[0])
    assert med == rmed[0, 0] and dmad == rmad[0, 0] and maths.mad(sig[0]) == dmad
    med, dmad = maths.med_mad(sig, axis=0, keepdims=True)
    rmed, rmad = ref_med_mad(sig, 0)
    assert med.shape == (1, 250) and np.allclose(med, rmed, rtol=1e-6) and np.allclose(dmad, rmad, rtol=1e-6)
    assert np.allclose(maths.mad(sig, factor=1.0), np.median(np.abs(sig - np.median(sig))), rtol=1e-6)


def test_chunkify_against_the_fixture(gold, tables):
    """Test 2: chunkify / chunkify_many, three normalisations: labels and bad equal, features within e_ref + e_dev; chunkify_many equals
    chunkify per read bit for bit."""
    need_gpu()
    from sloika_amd import batch
    batch.init_chunk_identity_worker(5, b"ACGT")
    bound = 2.0 * float(gold["e_ref"]) + float(np.spacing(np.float32(gold["max_abs"])))
    names = [n for n in ec.CASES if len(tables[n]) >= min(ec.CHUNK_LENS)]
    for cl in ec.CHUNK_LENS:
        reads = [n for n in names if len(tables[n]) >= cl]
        for norm in ec.NORMALISATIONS:
            many = batch.chunkify_many([tables[n] for n in reads], cl, 5, False, norm)
            for name, (mc, ml_, mb) in zip(reads, many):
                ev = tables[name]
                ml = len(ev) // cl
                chunks, labels, bad = batch.chunkify(ev, cl, 5, False, norm)
                assert chunks.shape == (ml, cl, 4) and chunks.dtype == np.float32
                assert labels.shape == (ml, cl) and labels.dtype == np.int32 and bad.shape == (ml, cl) and bad.dtype == np.bool_
                assert np.array_equal(mc, chunks) and np.array_equal(ml_, labels) and np.array_equal(mb, bad), (name, cl, norm)
                if "%s_labels_%d" % (name, cl) in gold:
                    assert np.array_equal(labels, gold["%s_labels_%d" % (name, cl)]), (name, cl)
                    assert np.array_equal(bad, gold["%s_bad_%d" % (name, cl)]), (name, cl)
                # 'none' / 'per-read' chunks are the leading rows of from_events (asserted on the reference when the fixture was made)
                key = {"none": name + "_fe_n0_k0", "per-read": name + "_fe_n1_k0", "per-chunk": "%s_chunks_%d" % (name, cl)}[norm]
                if key not in gold:
                    continue
                ref = gold[key] if norm == "per-chunk" else gold[key][:ml * cl].reshape(ml, cl, 4)
                if norm == "none":
                    assert np.array_equal(chunks, ref), (name, cl)
                else:
                    check_features(chunks, ref, bound, (name, cl, norm))
    # the scaled columns, and a table whose k-mers are str
    ev = tables["n401"]
    chunks, labels, _ = batch.chunkify(ev, 100, 5, True, "per-read")
    check_features(chunks, gold["n401_fe_scaled"][:400].reshape(4, 100, 4), bound, "scaled")
    as_str = {k: (ev[k].astype("U5") if k == "kmer" else ev[k]) for k in ev.dtype.names}
    assert np.array_equal(batch.chunkify(as_str, 100, 5, True, "per-read")[1], labels)
    # a shorter k-mer than the table's: the rightmost middle one (batch.py:69-73)
    batch.init_chunk_identity_worker(3, b"ACGT")
    try:
        lab3 = batch.chunkify(ev, 100, 3, False, "none")[1]
    finally:
        batch.init_chunk_identity_worker(5, b"ACGT")
    rank = {c: i for i, c in enumerate(b"ACGT")}
    want = np.asarray([1 + sum(rank[c] * 4 ** (2 - j) for j, c in enumerate(k[1:4])) for k in ev["kmer"][:400]]).reshape(4, 100)
    assert np.array_equal(lab3[labels != 0], want[labels != 0]) and np.array_equal(lab3 == 0, labels == 0)


def mixed_tables(tables):
    rs = np.random.RandomState(8)
    out = []
    for name, lo, hi in (("n2000", 0, 2000), ("n10750", 300, 1450), ("n401", 0, 401), ("n2000", 500, 1203), ("n7", 0, 7), ("n401", 7, 300)):
        out.append(tables[name][lo:hi].copy())
    rs.shuffle(out[0]["stdv"])
    return out


@pytest.mark.parametrize("model", ["tiny_gru", "baseline_lstm"])
def test_call_events_equals_the_worker_read_by_read(tables, model, capsys):
    """Test 3: tables of mixed length as one padded ragged batch: per read bit-identical to basecall.events_read_worker on that read
    alone; a table with nothing left after trimming and one with a value that is not finite are reported, the rest unaffected."""
    need_gpu()
    from sloika_amd import basecall, models, pipeline
    net = models.randomise_zero_layers(models.build_model(model, klen=5, sd=0.5, seed=5))
    calc_post = net.compile()
    bc = pipeline.Basecaller(net, kmer_len=5, min_prob=1e-5, skip=5.0)
    reads = mixed_tables(tables)
    for trim in ((0, 0), (3, 2)):
        scores, paths, lens, nev = bc.call_events(reads, trim=trim)
        scores, paths, lens = scores.cpu().numpy(), paths.cpu().numpy(), lens.cpu().numpy()
        assert nev == [len(r) - sum(trim) for r in reads]
        single = {}
        for b, r in enumerate(reads):
            name, score, call, n = basecall.events_read_worker(calc_post, r, trim=trim, kmer_len=5, min_prob=1e-5, skip=5.0, name="r%d" % b)
            assert n == nev[b] and name == "r%d" % b
            assert int(lens[b]) == len(call) and paths[b, :lens[b]].tolist() == [int(c) for c in call], (b, trim)
            assert (paths[b, lens[b]:] == -1).all()
            assert float(scores[b]) == float(score), (b, trim)
            single[b] = (float(score), call)
        # another order and composition: the same calls
        s2, p2, l2, _ = bc.call_events([reads[3], reads[0]], trim=trim)
        assert float(s2[1]) == single[0][0] and p2.cpu().numpy()[1, :int(l2[1])].tolist() == [int(c) for c in single[0][1]]
        assert float(s2[0]) == single[3][0]
    capsys.readouterr()
    broken = reads[2].copy()
    broken["mean"][17] = np.inf
    short = reads[4][:5]
    scores, paths, lens, nev = bc.call_events([reads[0], broken, reads[3], short, reads[2]], trim=(3, 2))
    err = capsys.readouterr().err
    assert "read 1" in err and "not finite" in err and "read 3" in err and "read 0" not in err and "read 2" not in err
    assert nev == [len(reads[0]) - 5, 0, len(reads[3]) - 5, 0, len(reads[2]) - 5]
    scores, paths, lens = scores.cpu().numpy(), paths.cpu().numpy(), lens.cpu().numpy()
    assert np.isnan(scores[[1, 3]]).all() and (lens[[1, 3]] == 0).all() and (paths[[1, 3]] == -1).all()
    for b, k in ((0, 0), (2, 3), (4, 2)):
        assert float(scores[b]) == single[k][0] and paths[b, :lens[b]].tolist() == [int(c) for c in single[k][1]]
    assert basecall.events_read_worker(calc_post, short, trim=(3, 2)) is None


def test_events_read_worker_against_the_float64_path(gold, tables):
    """Test 4: the features of the fixture (the reference's own float32 output) fed to net.compile() then decode_post give the same path
    as the worker, which makes its features on the device, on the same table."""
    need_gpu()
    from sloika_amd import basecall, models
    net = models.randomise_zero_layers(models.build_model("baseline_gru", klen=5, sd=0.5, seed=7))
    calc_post = net.compile()
    for name in ("n401", "n2000"):
        ev = tables[name]
        got = basecall.events_read_worker(calc_post, ev, trim=(0, 0), kmer_len=5, min_prob=1e-5, skip=5.0, name=name)
        post = calc_post(np.ascontiguousarray(gold[name + "_fe_n1_k0"][:, None, :]))
        score, call = basecall.decode_post(post, 5, True, True, 1e-5, skip=5.0)
        assert got[0] == name and got[3] == len(ev)
        assert [int(c) for c in got[2]] == [int(c) for c in call], name
        print("%s: worker score %.6f, score from the fixture's features %.6f" % (name, float(got[1]), float(score)))


def test_degenerate_shapes():
    """Test 5: a segment of one event (every deviation 0: all zeros, as the reference gives), one segment, 50 000 short segments in one
    launch -- each the bits it gets alone -- and a segment of more than a million events; seg_keep and the output pitch."""
    need_gpu()
    rs = np.random.RandomState(21)
    cols = np.stack([90 + 12 * rs.normal(size=1 << 20), np.abs(rs.normal(size=1 << 20)) + 0.5,
                     (rs.geometric(0.1, size=1 << 20) + 2).astype(np.float64)])
    one = kernel(cols, ([5], [1], [1], [0]), (1, 4), 4)
    assert np.array_equal(one, np.zeros((1, 4), dtype=np.float32))
    # 50 000 segments of 1 .. 40 events, overlapping, every one into its own rows; nothing else written
    nseg = 50000
    start = rs.randint(0, cols.shape[1] - 64, size=nseg)
    length = rs.randint(1, 41, size=nseg)
    keep = np.maximum(length - rs.randint(0, 3, size=nseg), 1)
    row = np.concatenate([[0], np.cumsum(keep + 1)[:-1]])                   # a row of slack behind every segment
    out = kernel(cols, (start, length, keep, row), (int((keep + 1).sum()), 4), 4)
    f32 = cols.astype(np.float32)
    for s in list(range(0, nseg, 997)) + [nseg - 1]:
        ev = {"mean": cols[0, start[s]:start[s] + length[s]], "stdv": cols[1, start[s]:start[s] + length[s]],
              "length": cols[2, start[s]:start[s] + length[s]]}
        want = ec.features64(ev, "", True, False)[:keep[s]]
        got = out[row[s]:row[s] + keep[s]]
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), s
        assert np.isnan(out[row[s] + keep[s]]).all(), s                      # the slack row is untouched
        alone = kernel(cols, ([start[s]], [length[s]], [keep[s]], [0]), (int(keep[s]), 4), 4)
        assert np.array_equal(alone, got), s
    # float32 columns give the same bits as their float64 copies
    assert np.array_equal(kernel(f32, ([100], [3000], [3000], [0]), (3000, 4), 4),
                          kernel(f32.astype(np.float64), ([100], [3000], [3000], [0]), (3000, 4), 4))
    # one long segment written with the pitch of a [T, B, 4] network input, column 2 of 3
    n = cols.shape[1] - 3
    big = kernel(cols, ([3], [n], [n], [2]), (n, 3, 4), 12, fill=0.0)
    want = ec.features64({"mean": cols[0, 3:], "stdv": cols[1, 3:], "length": cols[2, 3:]}, "", True, False)
    assert not big[:, :2].any()
    assert np.abs(big[:, 2] - want).max() <= 1e-6 * np.abs(want).max()
