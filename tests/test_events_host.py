"""The event front end, host side (no GPU): the fixture and its seeded inputs, argument checks of the new functions, the segment tables
batch.chunkify builds for slk_event_features_f32, the HDF5 compound-datatype decoder on bytes built by hand, and -- where a checkout of
the reference with its data/reads is at hand -- the two event counts its own test pins for Fast5.get_section_events."""
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import event_cases as ec  # noqa: E402

REF_READS = os.path.join(os.environ.get("SLOIKA_REFERENCE", "/root/reference"), "data", "reads")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "events.npz")))


def test_fixture_loads_and_its_inputs_regenerate(gold):
    for name, (n, _seed, _ft, _lt, const) in ec.CASES.items():
        cols = ec.columns(name)
        h = hashlib.sha256()
        for k in sorted(cols):
            h.update(np.ascontiguousarray(cols[k]).tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), gold[name + "_digest"]), \
            "%s: the regenerated table differs from the one the reference saw" % name
        assert gold[name + "_fe_n1_k0"].shape == (n, 4) and gold[name + "_fe_n1_k0"].dtype == np.float32
        if const is not None:
            assert not gold[name + "_fe_n1_k0"][:, 1].any()              # a deviation of exactly 0: x - m
    assert not gold["n1_fe_n1_k0"].any()                                 # one event: all zeros
    assert gold["n2000_chunks_500"].shape == (4, 500, 4) and gold["n10750_labels_500"].shape == (21, 500)
    assert gold["n401_labels_100"].dtype == np.int32 and gold["n401_bad_100"].dtype == np.bool_
    assert (gold["n401_labels_100"][:, 0] != 0).all() and (gold["n401_labels_100"] == 0).any()


def test_e_ref_is_the_references_distance_from_the_float64_evaluation(gold):
    """The stored e_ref, recomputed from the stored outputs and the float64 evaluation written in event_cases.py."""
    e_ref = max_abs = 0.0

    def measure(ref, f64):
        nonlocal e_ref, max_abs
        ok = np.isfinite(f64) & np.isfinite(ref)
        if ok.any():
            e_ref = max(e_ref, float(np.abs(ref.astype(np.float64) - f64)[ok].max()))
            max_abs = max(max_abs, float(np.abs(f64[ok]).max()))
    with np.errstate(all="ignore"):
        for name in ec.CASES:
            ev = ec.table(ec.columns(name))
            for normalise, nanonet in ((1, 0), (1, 1), (0, 1)):
                key = "%s_fe_n%d_k%d" % (name, normalise, nanonet)
                if key in gold:
                    f64 = ec.features64(ev, "", bool(normalise), bool(nanonet))
                    measure(gold[key] if normalise else gold[key][:, 3], f64 if normalise else f64[:, 3])
            if name + "_fe_scaled" in gold:
                measure(gold[name + "_fe_scaled"], ec.features64(ev, "scaled_", True, False))
            for cl in ec.CHUNK_LENS:
                if "%s_chunks_%d" % (name, cl) in gold:
                    measure(gold["%s_chunks_%d" % (name, cl)], ec.chunk_features64(ev, "", cl))
        x = ec.studentise_input()
        for key, axis in (("axis0", 0), ("axis1", 1), ("all", None)):
            measure(gold["studentise_" + key], ec.studentise64(x, axis))
    # (the generator also measured the outputs it did not store -- the biggest table's other variants -- which can only raise it)
    assert e_ref <= float(gold["e_ref"]) <= 2.0 * e_ref
    assert max_abs <= float(gold["max_abs"])
    assert float(gold["e_ref"]) < 1e-3 and float(gold["max_abs"]) < 20.0


def test_event_columns_and_their_checks():
    from sloika_amd import features
    ev = ec.table(ec.columns("n7"))
    cols = features.event_columns(ev, "")
    assert cols.shape == (3, 7) and cols.dtype == np.float64               # float32 columns, but an integer length
    assert np.array_equal(cols[0], ev["mean"].astype(np.float64)) and np.array_equal(cols[2], ev["length"])
    narrow = {"scaled_mean": ev["mean"], "scaled_stdv": ev["stdv"], "length": ev["length"].astype(np.float32)}
    assert features.event_columns(narrow).dtype == np.float32
    assert features.event_columns(ec.table(ec.columns("n2")), "scaled_").dtype == np.float64
    with pytest.raises(KeyError):
        features.event_columns(narrow, "")                                   # no 'mean' without the tag
    with pytest.raises(KeyError):
        features.event_columns({"mean": ev["mean"], "stdv": ev["stdv"]}, "")
    with pytest.raises(ValueError):
        features.event_columns({"mean": ev["mean"], "stdv": ev["stdv"][:3], "length": ev["length"]}, "")
    with pytest.raises(TypeError):
        features.event_columns({"mean": ev["kmer"], "stdv": ev["stdv"], "length": ev["length"]}, "")


def test_trim_ends_and_filter():
    from sloika_amd import batch
    ev = ec.table(ec.columns("n401"))
    assert batch.trim_ends_and_filter(ev, (50, 51), 0, 300) is not None
    assert len(batch.trim_ends_and_filter(ev, (50, 51), 0, 300)) == 300
    assert np.array_equal(batch.trim_ends_and_filter(ev, (50, 51), 0, 300)["mean"], ev["mean"][50:350])
    assert batch.trim_ends_and_filter(ev, (50, 52), 0, 300) is None        # shorter than sum(trim) + chunk_len
    assert batch.trim_ends_and_filter(ev, (0, 0), 402, 100) is None        # shorter than min_length
    assert len(batch.trim_ends_and_filter(ev, (0, 0), 401, 100)) == 401


@pytest.mark.parametrize("name", ["n401", "n2000", "n10750"])
@pytest.mark.parametrize("chunk_len", ec.CHUNK_LENS)
def test_segment_table_of_chunkify(name, chunk_len):
    """batch.py:37-60: per chunk, chunk_len + 1 events where the read has one more and chunk_len rows kept; otherwise the whole read."""
    from sloika_amd import batch
    nev = ec.CASES[name][0]
    if nev < chunk_len:
        with pytest.raises(ValueError):
            batch.event_segments(nev, chunk_len, "per-chunk")
        return
    ml = nev // chunk_len
    start, length, keep, row, normalise = batch.event_segments(nev, chunk_len, "per-chunk")
    assert normalise and all(a.dtype == np.int64 and a.shape == (ml,) for a in (start, length, keep, row))
    assert np.array_equal(start, np.arange(ml) * chunk_len) and np.array_equal(row, start) and (keep == chunk_len).all()
    assert (length[:-1] == chunk_len + 1).all()
    assert length[-1] == (chunk_len if nev % chunk_len == 0 else chunk_len + 1)     # the last chunk without / with the extra event
    assert (start + length <= nev).all()
    for norm, flag in (("none", False), ("per-read", True)):
        start, length, keep, row, normalise = batch.event_segments(nev, chunk_len, norm)
        assert (start.tolist(), length.tolist(), keep.tolist(), row.tolist(), normalise) == ([0], [nev], [ml * chunk_len], [0], flag)
    # inside a set of reads (chunkify_many): events and rows shifted
    start, length, keep, row, _ = batch.event_segments(nev, chunk_len, "per-chunk", first_event=1000, first_row=300)
    assert start[0] == 1000 and row[0] == 300 and start[-1] == 1000 + (ml - 1) * chunk_len
    with pytest.raises(ValueError):
        batch.event_segments(nev, chunk_len, "per-window")
    with pytest.raises(ValueError):
        batch.event_segments(chunk_len - 1, chunk_len, "none")


def test_worker_argument_checks(capsys):
    from sloika_amd import basecall

    def calc_post(x):
        raise AssertionError("the model must not be reached")
    args = ("no_such_file.fast5", "template", "Segment_Linear", (0, 0), 5)
    with pytest.raises(ValueError):
        basecall.events_worker(*args, True, True, 1e-5)                      # no compiled model
    for transducer, bad, trans in ((False, True, None), (True, False, None), (True, True, [0.1, 0.8, 0.1])):
        with pytest.raises(NotImplementedError):
            basecall.events_worker(*args, transducer, bad, 1e-5, trans=trans, calc_post=calc_post)
    assert basecall.events_worker(*args, True, True, 1e-5, calc_post=calc_post) is None      # basecall.py:73-75
    assert "Error getting events for section 'template'" in capsys.readouterr().err
    ev = ec.table(ec.columns("n7"))
    assert basecall.events_read_worker(calc_post, ev, trim=(4, 3), name="seven") is None      # basecall.py:78-80
    assert "Read too short in seven" in capsys.readouterr().err
    with pytest.raises(AssertionError):
        basecall.events_read_worker(calc_post, ev, trim=(-1, 0))


def _int_type(size, signed=True):
    return struct.pack("<BBBBI", 0x10, 0x08 if signed else 0, 0, 0, size) + struct.pack("<HH", 0, 8 * size)


def _float_type(size):
    props = {8: struct.pack("<HHBBBBI", 0, 64, 52, 11, 0, 52, 1023), 4: struct.pack("<HHBBBBI", 0, 32, 23, 8, 0, 23, 127)}[size]
    return struct.pack("<BBBBI", 0x11, 0x20, 63 if size == 8 else 31, 0, size) + props


def _string_type(size):
    return struct.pack("<BBBBI", 0x13, 0, 0, 0, size)


def _compound(version, members, size):
    """An HDF5 compound datatype message (File Format Specification, IV.A.2.d, class 6), written out by hand."""
    body = struct.pack("<BHBI", (version << 4) | 6, len(members), 0, size)
    for name, offset, mtype in members:
        raw = name.encode() + b"\0"
        if version < 3:
            raw += b"\0" * (-len(raw) % 8)
            body += raw + struct.pack("<I", offset)
            if version == 1:
                body += bytes(28)
        else:
            body += raw + struct.pack("<B", offset)
        body += mtype
    return body


@pytest.mark.parametrize("version", [1, 2, 3])
def test_compound_datatype_decoder(version):
    from sloika_amd import fast5
    members = [("start", 0, _int_type(8)), ("length", 8, _int_type(4, signed=False)), ("mean", 12, _float_type(8)),
               ("stdv", 20, _float_type(4)), ("model_state", 24, _string_type(5))]
    body = b"\xAA" * 3 + _compound(version, members, 32) + b"\xBB" * 5
    h5 = fast5.HDF5File.__new__(fast5.HDF5File)
    kind, dtype, size, used = h5._datatype(body, 3)
    assert kind == "compound" and size == 32 and dtype.itemsize == 32 and used == len(body) - 8
    assert dtype.names == ("start", "length", "mean", "stdv", "model_state")
    assert [dtype.fields[n][1] for n in dtype.names] == [0, 8, 12, 20, 24]
    assert [dtype[n].str for n in dtype.names] == ["<i8", "<u4", "<f8", "<f4", "|S5"]
    rows = np.zeros(3, dtype=dtype)
    rows["start"], rows["length"], rows["mean"], rows["stdv"] = [-5, 0, 7], [3, 4, 5], [80.5, 71.25, 99.0], [1.5, 0.5, 2.0]
    rows["model_state"] = [b"ACGTA", b"CG", b"TTTTT"]
    back = h5._decode(kind, dtype, size, (3,), rows.tobytes())
    assert back.dtype == dtype and np.array_equal(back, rows)
    # what the decoder does not read is refused, not guessed
    nested = _compound(version, [("inner", 0, _compound(version, members[:1], 8))], 8)
    with pytest.raises(fast5.Fast5Error):
        h5._datatype(nested)
    if version == 1:
        arr = bytearray(_compound(1, members[:1], 8))
        arr[8 + 8 + 4] = 1                                                   # dimensionality of the first member
        with pytest.raises(fast5.Fast5Error):
            h5._datatype(bytes(arr))


@pytest.mark.parametrize("read,count", [("read3.fast5", 9946), ("read6.fast5", 11145)])
def test_section_events_of_the_references_reads(read, count):
    """The only pin there is for Fast5.get_section_events: the reference's own test (test/unit/test_fast5.py:81-90)."""
    path = os.path.join(REF_READS, read)
    if not os.path.exists(path):
        pytest.skip("the reference's data/reads is not on this machine")
    from sloika_amd import fast5
    f5 = fast5.Fast5(path)
    ev = f5.get_section_events("template", analysis="Segment_Linear")
    assert len(ev) == count
    assert ev.dtype.names == ("start", "length", "mean", "stdv") and all(ev.dtype[n] == np.float64 for n in ev.dtype.names)
    whole = f5.get_events()
    assert len(whole) == count + 5 and np.array_equal(whole[5:], ev)
    assert np.allclose(whole["start"][1:], whole["start"][:-1] + whole["length"][:-1])       # seconds, tiling the time axis
    assert 0.0002 <= whole["length"].min() and whole["length"].max() < 1.0
    with pytest.raises(ValueError):
        f5.get_section_events("complement")
    with pytest.raises(ValueError):
        f5.get_section_events("hairpin")
    with pytest.raises(fast5.Fast5Error):
        f5.get_section_events("template", analysis="Segment_Nowhere")
