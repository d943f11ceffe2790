"""The fixture of `chunkify remap` for event models (tests/golden/event_remap.npz, made by the reference's own batch.remap and
batch.chunkify) against the numpy restatement the GPU tests compare the label kernel with, and the host-only ends of
sloika_amd.batch's remap interface.  No GPU."""
import numpy as np
import pytest

from tests import event_remap_ref as er
from tests.event_remap_ref import erc


@pytest.mark.parametrize("name", erc.NAMES)
def test_restatement_reproduces_the_fixture(name):
    g, c = er.gold(), er.case(name)
    path, seq = g[name + "_path"], g[name + "_seq"]
    assert list(seq) == list(c["states"]) and len(path) == c["nev"] and int(g[name + "_masked"]) == 0
    labels = er.labels_of_path(path, seq, c["chunk_len"])
    assert labels.dtype == np.int32 and np.array_equal(labels, g[name + "_labels"])
    assert not g[name + "_bad"].any() and g[name + "_bad"].shape == labels.shape
    nstay, start, end = er.strand_stats(path)
    assert [str(nstay), str(len(seq)), str(start), str(end)] == g[name + "_strand"][3:].tolist()
    # the appended columns are the path, the k-mers under it, and True
    assert np.array_equal(g[name + "_seq_pos"], path) and g[name + "_good"].all()
    kmers = np.asarray([c["ref"][p:p + c["k"]] for p in range(len(seq))], dtype="S%d" % c["k"])
    assert np.array_equal(g[name + "_kmer"], kmers[path])


@pytest.mark.parametrize("name", erc.NAMES)
def test_paths_show_what_the_cases_name(name):
    assert erc.unmet(er.case(name), er.gold()[name + "_path"]) == []


def test_cases_cover_what_the_kernels_can_get_wrong():
    cs = [erc.CASES[n] for n in erc.NAMES]
    assert {3, 5} <= {c["k"] for c in cs} and {1, 7, 100} <= {c["chunk_len"] for c in cs}
    assert {(None, None), (25.0, 25.0)} <= {tuple(c["prior"]) for c in cs}
    for need in ("jump", "stay_on_chunk_start", "all_stay"):
        assert any(c["needs"].get(need) for c in cs), need
    for cl in (7, 100):
        rest = {c["needs"]["remainder"] == 0 for c in cs if c["chunk_len"] == cl}
        assert rest == {True, False}, cl


@pytest.mark.parametrize("name", erc.NAMES)
def test_strand_list_row_formats_the_fixture(name):
    from sloika_amd import batch
    g = er.gold()
    score = np.float32(float.fromhex(str(g[name + "_score_hex"])))
    assert score == g[name + "_score"]
    path, seq = g[name + "_path"], [int(v) for v in g[name + "_seq"]]
    result = (name + ".fast5", score, len(path), path, seq, g[name + "_chunks"], g[name + "_labels"], g[name + "_bad"])
    want = g[name + "_strand"].tolist()
    assert [str(x) for x in batch.strand_list_row(result)] == want
    assert [str(x) for x in batch.strand_list_row(result, stats=er.strand_stats(path))] == want


def test_training_takes_the_fixture_chunks():
    """What chunkify gives for remapped reads is what the training loop's data preparation takes (bin/train_network.py:207-252)."""
    from sloika_amd import train
    g = er.gold()
    names = [n for n in erc.NAMES if erc.CASES[n]["chunk_len"] == 100]
    chunks = np.concatenate([g[n + "_chunks"] for n in names])
    labels = np.concatenate([g[n + "_labels"] for n in names])
    bad = np.concatenate([g[n + "_bad"] for n in names])
    assert chunks.shape == (10, 100, 4) and chunks.dtype == np.float32
    data = {"chunks": chunks, "labels": labels, "bad": bad, "weights": np.ones(len(chunks))}
    all_labels, all_weights, label_weights = train.prepare_training_data(data)
    assert np.array_equal(all_labels, labels) and all_labels.dtype == np.int32
    assert all_weights.sum() == pytest.approx(1.0) and len(label_weights) == labels.max() + 1
    np.random.seed(3)
    indata, lab, weights, rate = next(train.training_batches(chunks, all_labels, all_weights, label_weights, 1, batch_size=4,
                                                             drop=5))
    assert indata.shape[1:] == (4, 4) and indata.dtype == np.float32 and lab.shape[1] == 4


def test_remap_refuses_what_it_cannot_do():
    from sloika_amd import batch
    c = er.case("k3_cl7_rest")
    keep = batch.calc_post
    batch.calc_post = None
    try:
        with pytest.raises(ValueError, match="compiled model"):
            batch.remap(c["ref"], c["ev"], 1e-5, 3, (None, None), 5.0)
        with pytest.raises(ValueError, match="network"):
            batch.remap_many([c["ref"]], [c["ev"]], 1e-5, 3, (None, None), 5.0)
    finally:
        batch.calc_post = keep
    # a table that already has one of the columns: numpy's own complaint, before anything runs
    import numpy.lib.recfunctions as nprf
    twice = nprf.append_fields(c["ev"], ["seq_pos"], [np.zeros(len(c["ev"]), "i4")], usemask=False)
    with pytest.raises(ValueError) as numpys:
        nprf.append_fields(twice, ["seq_pos", "kmer", "good_emission"],
                           [np.zeros(len(twice), "i4"), np.zeros(len(twice), "S3"), np.ones(len(twice), "?")])
    with pytest.raises(ValueError) as ours:
        batch.remap(c["ref"], twice, 1e-5, 3, (None, None), 5.0, calc_post=lambda x: x)
    assert str(ours.value) == str(numpys.value)


def test_worker_reports_like_the_reference(capsys):
    """The three stderr messages of batch.py:163-185, none of which needs a device."""
    from sloika_amd import batch
    c = er.case("k3_cl7_rest")

    class Read(object):
        filename_short = "read7"

        def __init__(self, ev):
            self.ev = ev

        def get_section_events(self, section, analysis=None):
            if self.ev is None:
                raise ValueError("no %s section by %s" % (section, analysis))
            return self.ev

        def __repr__(self):
            return "read7.fast5"

    args = ((1, 1), 1e-5, 3, (None, None), 5.0, 7, False, "per-read", 10, "template", "Segment_Linear")
    assert batch.chunk_remap_worker(Read(None), *args, {"read7": c["ref"]}) is None
    err = capsys.readouterr().err
    assert err.startswith("Failure reading events from read7.fast5.\n") and "no template section by Segment_Linear" in err
    assert batch.chunk_remap_worker(Read(c["ev"]), *args, {}) is None
    assert capsys.readouterr().err == "No reference found for read7.fast5.\n%r\n" % KeyError("read7")
    assert batch.chunk_remap_worker(Read(c["ev"][:8]), *args, {"read7": c["ref"]}) is None          # 8 < 1 + 1 + 7
    assert capsys.readouterr().err == "read7.fast5 is too short.\n"
    assert batch.chunk_remap_worker("/no/such/file.fast5", *args, {}) is None
    assert capsys.readouterr().err.startswith("Failure reading events from /no/such/file.fast5.\n")
