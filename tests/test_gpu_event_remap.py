"""`chunkify remap` for event models on the GPU: the two kernels of csrc/event_remap.hip through the C ABI, and batch.remap /
remap_many / chunk_remap_worker / chunk_remap_many, against the outputs of the reference's own batch.remap and batch.chunkify
(tests/golden/event_remap.npz) and against each other.

Bounds.  Integers (paths, labels, columns, strand statistics) and everything compared device against device are exact.  A score
against the fixture gets the relative 2e-6 tests/test_gpu_chunkify_raw.py gives a log=False remap (design/remap.md: the last bit of
a float32 log).  Chunks against the fixture get e_ref + e_dev of tests/golden/events.npz as tests/test_gpu_events.py spends it on the
host interface: e_dev <= e_ref + one float32 ulp of the largest studentised magnitude there."""
import os

import numpy as np
import pytest

from tests import event_remap_ref as er
from tests.event_remap_ref import erc
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

CANARY = -12345.0
ICANARY = -777


@pytest.fixture()
def worker_state():
    """The process globals the remap interface reads, put back afterwards."""
    from sloika_amd import batch
    keep = batch.kmer_to_state, batch.kmer_alphabet, batch.calc_post
    yield batch
    batch.kmer_to_state, batch.kmer_alphabet, batch.calc_post = keep


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- slk_remap_pack_log_post_f32 -----------------------------------------------------------------------------------------------------

def prepare_then_log(rows, min_prob):
    """slk_prepare_post_f32 followed by slk_log_post_f32(POST_LN) on one read's rows alone."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    src = rows.contiguous()
    mid, out = torch.empty_like(src), torch.empty_like(src)
    if src.numel():
        assert L.slk_prepare_post_f32(src.data_ptr(), mid.data_ptr(), src.numel(), min_prob, stream()) == 0
        assert L.slk_log_post_f32(mid.data_ptr(), out.data_ptr(), mid.numel(), _lib.POST_LN, 0.0, stream()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("S,steps,wide", [(65, (1, 37, 64), False), (1025, (1, 37, 64), False), (65, (1, 37, 64), True),
                                          (1025, (1, 37, 64), True), (65, (64, 0, 37), False), (1025, (37, 0, 1), True)])
def test_pack_equals_prepare_and_log_per_read(S, steps, wide):
    torch = need_gpu()
    from sloika_amd import _lib
    T, B, min_prob = 64, 3, 1e-5
    rs = np.random.RandomState(S + sum(steps) + wide)
    ld = S + 7 if wide else S                                  # a batch stride wider than the row
    store = torch.full((T, B, ld), float("nan"), dtype=torch.float32, device="cuda")
    post = store[:, :, :S]
    post.copy_(dev(rs.dirichlet(np.ones(S) * 0.05, size=(T, B)).astype(np.float32)))
    for b, n in enumerate(steps):                              # steps at or beyond a read's count are not read
        post[n:, b, :] = float("nan")
    # every read owns two rows more than it has steps: they, and the canaries round `out`, stay as they were
    room = [n + 2 for n in steps]
    ev_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    pad = 3                                                    # (an `out` that does not start on a 16-byte boundary)
    whole = torch.full((pad + int(ev_off[-1]) * S + pad,), CANARY, dtype=torch.float32, device="cuda")
    out = whole[pad:pad + int(ev_off[-1]) * S]
    nstep_d, ev_d = dev(np.asarray(steps, dtype=np.int32)), dev(ev_off)          # (named: they must outlive the launch)
    rc = _lib.lib().slk_remap_pack_log_post_f32(post.data_ptr(), post.stride(0), post.stride(1), T, B, S, nstep_d.data_ptr(),
                                                ev_d.data_ptr(), min_prob, out.data_ptr(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert (got[:pad] == CANARY).all() and (got[-pad:] == CANARY).all()
    got = got[pad:-pad].reshape(-1, S)
    for b, n in enumerate(steps):
        want = prepare_then_log(post[:n, b, :], min_prob)
        mine = got[ev_off[b]:ev_off[b] + n]
        assert np.isfinite(mine).all() and np.array_equal(bits(mine), bits(want)), (b, n)
        assert (got[ev_off[b] + n:ev_off[b + 1]] == CANARY).all(), (b, n)


# ---- slk_event_remap_labels_i32 ------------------------------------------------------------------------------------------------------

def label_kernel(paths, seqs, chunk_len):
    """The kernel on a ragged set, canaries round every output: -> (labels per read, stats [n, 3], status)."""
    torch = need_gpu()
    from sloika_amd import _lib
    n = len(paths)
    ev_off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    pos_off = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.int64)
    rows = [(len(p) // chunk_len) * chunk_len for p in paths]
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    total, pad = int(row_off[-1]), 5
    labels = torch.full((pad + total + pad,), ICANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((pad + 3 * n + pad,), ICANARY, dtype=torch.int32, device="cuda")
    status = torch.full((3,), ICANARY, dtype=torch.int32, device="cuda")
    status[1] = 0
    # (named: the inputs must outlive the launch)
    path_d, seq_d = dev(np.concatenate(paths).astype(np.int32)), dev(np.concatenate(seqs).astype(np.int32))
    ev_d, pos_d, row_d = dev(ev_off), dev(pos_off), dev(row_off)
    rc = _lib.lib().slk_event_remap_labels_i32(path_d.data_ptr(), ev_d.data_ptr(), seq_d.data_ptr(), pos_d.data_ptr(), n, chunk_len,
                                               row_d.data_ptr(), total, labels[pad:].data_ptr(), stats[pad:].data_ptr(),
                                               status[1:].data_ptr(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    labels, stats, status = labels.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()
    for a in (labels, stats):
        assert (a[:pad] == ICANARY).all() and (a[-pad:] == ICANARY).all()
    assert status[0] == ICANARY and status[2] == ICANARY
    labels = labels[pad:-pad]
    return ([labels[row_off[r]:row_off[r + 1]].reshape(-1, chunk_len) for r in range(n)], stats[pad:-pad].reshape(n, 3), int(status[1]))


@pytest.mark.parametrize("name", erc.NAMES)
def test_label_kernel_on_the_fixture(name):
    g, cl = er.gold(), erc.CASES[name]["chunk_len"]
    path, seq = g[name + "_path"], g[name + "_seq"]
    labels, stats, status = label_kernel([path], [seq], cl)
    assert status == 0
    assert np.array_equal(labels[0], er.labels_of_path(path, seq, cl)) and np.array_equal(labels[0], g[name + "_labels"])
    assert tuple(stats[0]) == er.strand_stats(path)
    assert [str(v) for v in stats[0]] == [g[name + "_strand"][i] for i in (3, 5, 6)]


@pytest.mark.parametrize("chunk_len", [1, 7, 100])
def test_label_kernel_on_a_ragged_set(chunk_len):
    """All fixture paths long enough for the chunk length in one launch, the smallest read there can be (one chunk) first and last."""
    g = er.gold()
    names = [n for n in erc.NAMES if erc.CASES[n]["nev"] >= chunk_len]
    rs = np.random.RandomState(chunk_len)
    small_seq = rs.randint(1, 65, size=3)
    small = rs.randint(0, 3, size=chunk_len)
    paths = [small] + [g[n + "_path"] for n in names] + [small[::-1].copy()]
    seqs = [small_seq] + [g[n + "_seq"] for n in names] + [small_seq]
    labels, stats, status = label_kernel(paths, seqs, chunk_len)
    assert status == 0
    for r, (p, q) in enumerate(zip(paths, seqs)):
        assert np.array_equal(labels[r], er.labels_of_path(p, q, chunk_len)), r
        assert tuple(stats[r]) == er.strand_stats(p), r
    assert labels[0].shape == (1, chunk_len) and max(len(p) for p in paths) == 700


def test_label_kernel_flags_a_position_outside_the_reference():
    g = er.gold()
    name = "k3_cl7_rest"
    path, seq = g[name + "_path"].copy(), g[name + "_seq"]
    path[10] = len(seq)                                        # one past the last position
    path[44] = -1                                              # (beyond the label rows: 45 events, six chunks of 7)
    labels, stats, status = label_kernel([g[name + "_path"], path], [seq, seq], 7)
    assert status == 2
    assert np.array_equal(labels[0], g[name + "_labels"])      # the read beside it is unaffected
    pos = path[:42].astype(np.int64).reshape(6, 7)
    outside = (pos < 0) | (pos >= len(seq))
    want = seq[np.where(outside, 0, pos)].astype(np.int32)
    want[outside] = -1
    want[:, 1:][pos[:, 1:] == pos[:, :-1]] = 0
    assert want[1, 3] == -1 and outside.sum() == 1
    assert np.array_equal(labels[1], want)
    assert tuple(stats[1]) == er.strand_stats(path)


# ---- batch.remap against the reference ------------------------------------------------------------------------------------------------

def stub_network(post):
    """The compiled model of the fixture: returns the case's posterior whatever the features (make_event_remap_goldens.py)."""
    def calc_post(inmat):
        assert tuple(inmat.shape[1:]) == (1, 4) and inmat.shape[0] == len(post)
        return dev(post[:, None, :])
    return calc_post


@pytest.mark.parametrize("name", erc.NAMES)
def test_remap_matches_the_reference(name, worker_state):
    need_gpu()
    batch = worker_state
    g, c = er.gold(), er.case(name)
    ev_gold = dict(np.load(os.path.join(er.GOLD, "events.npz")))
    bound = 2.0 * float(ev_gold["e_ref"]) + float(np.spacing(np.float32(ev_gold["max_abs"])))      # e_ref + (e_dev <= e_ref + ulp)
    batch.init_chunk_identity_worker(c["k"], erc.ALPHABET)
    score, ev, path, seq = batch.remap(c["ref"], c["ev"], erc.MIN_PROB, c["k"], c["prior"], c["slip"], calc_post=stub_network(c["post"]))
    assert np.array_equal(path, g[name + "_path"]) and path.dtype == g[name + "_path"].dtype
    assert list(seq) == list(g[name + "_seq"])
    assert type(ev) is np.ndarray and ev.dtype.names == c["ev"].dtype.names + ("seq_pos", "kmer", "good_emission")
    for f, key in (("seq_pos", "_seq_pos"), ("kmer", "_kmer"), ("good_emission", "_good")):
        assert ev[f].dtype == g[name + key].dtype and np.array_equal(ev[f], g[name + key]), f
    for f in c["ev"].dtype.names:
        assert np.array_equal(ev[f], c["ev"][f]), f
    print("%s: score %r, the reference's %r" % (name, float(score), float(g[name + "_score"])))
    assert np.asarray(score).dtype == np.float32
    assert float(score) == pytest.approx(float(g[name + "_score"]), rel=2e-6)
    chunks, labels, bad = batch.chunkify(ev, c["chunk_len"], c["k"], c["use_scaled"], c["normalisation"])
    assert labels.dtype == np.int32 and np.array_equal(labels, g[name + "_labels"])
    assert bad.dtype == np.bool_ and np.array_equal(bad, g[name + "_bad"])
    want = g[name + "_chunks"]
    assert chunks.shape == want.shape and chunks.dtype == np.float32
    worst = float(np.abs(chunks.astype(np.float64) - want.astype(np.float64)).max())
    print("%s: chunks differ by at most %.3e, bound %.3e" % (name, worst, bound))
    assert worst <= bound


# ---- remap_many / chunk_remap_many against the single-read functions ---------------------------------------------------------------------

def random_reads():
    """Three event tables of 50, 333 and 120 events with references of 20, 200 and 90 bases."""
    rs = np.random.RandomState(41)
    big, other = er.case("k5_cl100_exact")["ev"], er.case("k5_cl100_rest")["ev"]
    evs = [big[100:150].copy(), other.copy(), big[400:520].copy()]
    refs = [bytes(rs.choice(list(erc.ALPHABET), size=n).tolist()) for n in (20, 200, 90)]
    return refs, evs


@pytest.fixture(scope="module")
def tiny_gru():
    need_gpu()
    from sloika_amd import models
    return models.randomise_zero_layers(models.build_model("tiny_gru", klen=5, sd=0.5, seed=5))


def same_result(a, b):
    assert len(a) == len(b) == 8 and a[0] == b[0] and a[2] == b[2]
    assert bits(a[1]) == bits(b[1]), (a[1], b[1])
    assert np.array_equal(a[3], b[3]) and a[3].dtype == b[3].dtype and list(a[4]) == list(b[4])
    for k in (5, 6, 7):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
    assert np.array_equal(bits(a[5]), bits(b[5])) and np.array_equal(a[6], b[6]) and np.array_equal(a[7], b[7])


def test_remap_many_equals_remap_read_by_read(tiny_gru, worker_state):
    batch = worker_state
    batch.init_chunk_identity_worker(5, erc.ALPHABET)
    refs, evs = random_reads()
    calc_post = tiny_gru.compile()
    for prior, slip in (((25.0, 25.0), 5.0), ((None, None), 2.5)):
        many = batch.remap_many(refs, evs, 1e-5, 5, prior, slip, network=tiny_gru)
        assert len(many) == 3
        for ref, ev, (score, table, path, seq) in zip(refs, evs, many):
            s1, t1, p1, q1 = batch.remap(ref, ev, 1e-5, 5, prior, slip, calc_post=calc_post)
            assert np.isfinite(score) and bits(score) == bits(s1), (score, s1)
            assert np.array_equal(path, p1) and path.dtype == p1.dtype and len(path) == len(ev)
            assert list(seq) == list(q1) and len(seq) == len(ref) - 4
            assert table.dtype == t1.dtype and np.array_equal(table, t1)
    # another order and composition: the same answers
    again = batch.remap_many(refs[::-1], evs[::-1], 1e-5, 5, (None, None), 2.5, network=tiny_gru)
    for (sa, _, pa, _), (sb, _, pb, _) in zip(again[::-1], many):
        assert bits(sa) == bits(sb) and np.array_equal(pa, pb)
    # the process-global model, as the reference's worker finds it
    batch.init_chunk_remap_worker(tiny_gru, 5, erc.ALPHABET)
    glob = batch.remap_many(refs[:1], evs[:1], 1e-5, 5, (None, None), 2.5)
    assert bits(glob[0][0]) == bits(many[0][0]) and np.array_equal(glob[0][2], many[0][2])


def test_remap_many_names_the_read_it_cannot_map(tiny_gru, worker_state):
    batch = worker_state
    batch.init_chunk_identity_worker(5, erc.ALPHABET)
    refs, evs = random_reads()
    with pytest.raises(ValueError, match="read 1 .*2 positions"):
        batch.remap_many([refs[0], b"ACGTAC", refs[2]], evs, 1e-5, 5, (None, None), 5.0, network=tiny_gru)
    too_long = (b"ACGT" * 1463)[:5851]                         # 5847 positions: one more than the DP's LDS holds
    with pytest.raises(ValueError, match="read 2 .*5847 positions"):
        batch.remap_many([refs[0], refs[1], too_long], evs, 1e-5, 5, (None, None), 5.0, network=tiny_gru)
    with pytest.raises(ValueError, match="read 0 .*no events"):
        batch.remap_many(refs, [evs[0][:0], evs[1], evs[2]], 1e-5, 5, (None, None), 5.0, network=tiny_gru)
    broken = evs[2].copy()
    broken["stdv"][5] = np.nan
    with pytest.raises(ValueError, match="read 2 .*not finite"):
        batch.remap_many(refs, [evs[0], evs[1], broken], 1e-5, 5, (None, None), 5.0, network=tiny_gru)


class StandIn(object):
    """What chunk_remap_worker reads of a fast5 file."""

    def __init__(self, name, ev):
        self.filename_short, self.ev = name, ev

    def get_section_events(self, section, analysis=None):
        assert section == "template" and analysis == "Segment_Linear"
        return self.ev

    def __repr__(self):
        return self.filename_short


@pytest.mark.parametrize("chunk_len,use_scaled,normalisation", [(7, True, "per-chunk"), (20, False, "per-read")])
def test_chunk_remap_many_equals_the_worker_loop(tiny_gru, worker_state, capsys, chunk_len, use_scaled, normalisation):
    batch = worker_state
    batch.init_chunk_remap_worker(tiny_gru, 5, erc.ALPHABET)
    refs, evs = random_reads()
    names = ["r0", "short", "r1", "orphan", "r2"]
    tables = [evs[0], evs[2][:chunk_len + 4], evs[1], evs[0], evs[2]]
    references = {"r0": refs[0], "short": refs[2], "r1": refs[1], "r2": refs[2]}
    args = ((3, 2), 1e-5, 5, (25.0, 25.0), 5.0, chunk_len, use_scaled, normalisation, 40)
    capsys.readouterr()
    single = [batch.chunk_remap_worker(StandIn(n, t), *args, "template", "Segment_Linear", references) for n, t in zip(names, tables)]
    err_single = capsys.readouterr().err
    results, strand = batch.chunk_remap_many(tables, names, references, *args)
    err_many = capsys.readouterr().err
    assert err_single == err_many == "short is too short.\nNo reference found for orphan.\n%r\n" % KeyError("orphan")
    assert [r is None for r in results] == [r is None for r in single] == [False, True, False, True, False]
    for one, many, st in zip(single, results, strand):
        if one is None:
            assert many is None and st is None
            continue
        same_result(one, many)
        assert many[2] == len(many[3]) and many[5].shape == (many[2] // chunk_len, chunk_len, 4) and not many[7].any()
        assert st == er.strand_stats(many[3])
        assert [str(x) for x in batch.strand_list_row(many, st)] == [str(x) for x in batch.strand_list_row(one)]
    # the others do not depend on who is beside them
    alone, st = batch.chunk_remap_many([tables[2]], ["r1"], references, *args)
    same_result(alone[0], results[2])
    assert st[0] == strand[2]
