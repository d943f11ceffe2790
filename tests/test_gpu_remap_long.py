"""The tiled remap DP (map_to_sequence_long_body, csrc/transducer.hip; design/remap_long.md): references of any length, one tile of
positions in LDS at a time.  Bit for bit on score and path against what the REFERENCE returned -- tests/golden/remap_slips.npz at
tiles of 64 and 128 positions, where reads of a few hundred positions reach every tile edge, and tests/golden/remap_long.npz
(tests/test_oracle_remap_long.py keeps that fixture honest without a GPU) -- and, on seeded reads, against the oracle that both
fixtures pin.  Outputs and workspace sit inside canaries."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle_remap
from tests.gpu_util import need_gpu
from tests.test_gpu_event_remap import random_reads, tiny_gru, worker_state       # noqa: F401  (fixtures)
from tests.test_gpu_remap_slips import (CANARY, PAD, SCORE_CANARY, _big_next_to_small, _bits, _canary, _dev, _GROUPS,
                                        _outside_untouched, _plain, _ptr, _same)
from tests.test_oracle_remap_long import lc, long_case
from tests.test_oracle_remap_slips import rc, slip_case

pytestmark = pytest.mark.gpu


def _words(nev, npos):
    """int32 elements of a read's workspace: the traceback and two score rows of npos + 16."""
    return nev * npos + 2 * (npos + 16)


def _ws_words(nev, npos, tile=0):
    from sloika_amd import _lib
    return _lib.lib().slk_map_to_sequence_long_workspace_bytes(nev, npos, tile) // 4


def _single_long(c, tile, short_by=0):
    """slk_map_to_sequence_long_f32 with path_out and the workspace inside canaries -> (rc, score, path, untouched outside, whether the
    workspace and the path were left as they were)."""
    import torch
    from sloika_amd import _lib, device as D
    nev, npos = len(c["ltrans"]), len(c["seq"])
    lt, seq, pi, pf = _dev(c["ltrans"]), _dev(c["seq"]), _dev(c["pi"]), _dev(c["pf"])
    nws = 4 * _words(nev, npos)
    if tile == 0 or (64 <= tile <= 6784 and tile % 64 == 0):
        assert _lib.lib().slk_map_to_sequence_long_workspace_bytes(nev, npos, tile) == nws
    ws, path = _canary(nws // 4), _canary(nev)
    score = torch.full((1,), float(SCORE_CANARY), dtype=torch.float32, device="cuda")
    rc_ = _lib.lib().slk_map_to_sequence_long_f32(_ptr(lt), nev, c["ltrans"].shape[1], _ptr(seq), npos, float(c["slip"]), _ptr(pi),
                                                  _ptr(pf), _ptr(ws, PAD), nws - short_by, tile, _ptr(score), _ptr(path, PAD),
                                                  D.stream_ptr())
    torch.cuda.synchronize()
    untouched = _outside_untouched(path, nev) and _outside_untouched(ws, nws // 4)
    nothing = bool((ws == CANARY).all()) and bool((path == CANARY).all()) and float(score.item()) == float(SCORE_CANARY)
    return rc_, np.float32(score.item()), path.cpu().numpy()[PAD:PAD + nev], untouched, nothing


class LongBatch(object):
    """Reads laid out for slk_map_to_sequence_long_batch_f32, uploaded once; the outputs sit inside canaries."""

    def __init__(self, reads, pi=False, pf=False):
        self.nev = [len(r["ltrans"]) for r in reads]
        self.npos = [len(r["seq"]) for r in reads]
        self.nst = reads[0]["ltrans"].shape[1]
        self.ev_off = np.concatenate([[0], np.cumsum(self.nev)]).astype(np.int64)
        pos_off = np.concatenate([[0], np.cumsum(self.npos)]).astype(np.int64)
        self.ws_words = np.asarray([_words(e, p) for e, p in zip(self.nev, self.npos)], dtype=np.int64)
        self.ws_off = np.concatenate([[0], np.cumsum(self.ws_words)[:-1]]).astype(np.int64)
        self.nws = int(self.ws_words.sum())
        self.lt = _dev(np.concatenate([r["ltrans"].reshape(-1, self.nst) for r in reads]))
        self.seq = _dev(np.concatenate([r["seq"] for r in reads]).astype(np.int32))
        self.pi = _dev(np.concatenate([r["pi"] for r in reads])) if pi else None
        self.pf = _dev(np.concatenate([r["pf"] for r in reads])) if pf else None
        self.off = [_dev(a) for a in (self.ev_off, pos_off, self.ws_off)]

    def run(self, slip, tile):
        import torch
        from sloika_amd import _lib, device as D
        nread = len(self.nev)
        self.ws = _canary(self.nws)
        self.path = _canary(int(self.ev_off[-1]))
        self.score = torch.full((nread,), float(SCORE_CANARY), dtype=torch.float32, device="cuda")
        rc_ = _lib.lib().slk_map_to_sequence_long_batch_f32(
            _ptr(self.lt), self.nst, _ptr(self.off[0]), _ptr(self.seq), _ptr(self.off[1]), nread, max(self.npos), float(slip),
            _ptr(self.pi), _ptr(self.pf), _ptr(self.ws, PAD), _ptr(self.off[2]), tile, _ptr(self.score), _ptr(self.path, PAD),
            D.stream_ptr())
        torch.cuda.synchronize()
        ph = self.path.cpu().numpy()[PAD:]
        return rc_, self.score.cpu().numpy(), [ph[self.ev_off[b]:self.ev_off[b + 1]] for b in range(nread)]

    def outside_untouched(self):
        return _outside_untouched(self.path, int(self.ev_off[-1])) and _outside_untouched(self.ws, self.nws)

    def nothing_written(self):
        return (bool((self.ws == CANARY).all()) and bool((self.path == CANARY).all())
                and bool((self.score == float(SCORE_CANARY)).all()))


# ---- 1, 2: the slip fixture at tiles that put an edge inside every read ----------------------------------------------------------------

@pytest.mark.parametrize("tile", [64, 128, 0])
def test_slip_fixture_through_the_single_entry(tile):
    need_gpu()
    from sloika_amd import _lib
    bad = []
    for name in rc.NAMES:
        c = slip_case(name)
        rc_, score, path, untouched, _ = _single_long(c, tile)
        assert rc_ == _lib.SLK_OK and untouched, name
        if not _same(score, path, c):
            bad.append((name, float(score), float(c["score"]), np.flatnonzero(path != c["path"])[:4].tolist()))
    assert not bad, bad


@pytest.mark.parametrize("nst,slip", _GROUPS)
def test_slip_fixture_batch_with_a_read_without_events_in_the_middle(nst, slip):
    need_gpu()
    from sloika_amd import _lib
    cases = _big_next_to_small([slip_case(n) for n in rc.NAMES
                                if _plain(n) and (rc.CASES[n]["gen"]["nst"], rc.CASES[n]["slip"]) == (nst, slip)])
    mid = len(cases) // 2
    empty = dict(ltrans=np.zeros((0, nst), dtype=np.float32), seq=cases[0]["seq"][:7])
    reads = cases[:mid] + [empty] + cases[mid:]
    for tile in (64, 0):
        b = LongBatch(reads)
        rc_, scores, paths = b.run(slip, tile)
        assert rc_ == _lib.SLK_OK and b.outside_untouched()
        assert scores[mid] == -np.inf and len(paths[mid]) == 0
        ws = b.ws.cpu().numpy()[PAD:]
        assert (ws[b.ws_off[mid]:b.ws_off[mid] + b.ws_words[mid]] == CANARY).all(), "the empty read's workspace was written"
        for r, c in enumerate(reads):
            if r != mid:
                assert _same(scores[r], paths[r], c), (tile, c["name"])


def test_read_with_two_positions_in_a_batch_is_left_alone():
    need_gpu()
    from sloika_amd import _lib
    left, right = slip_case("bt_last"), slip_case("nev_33")
    middle = dict(ltrans=right["ltrans"][:5], seq=left["seq"][:2])
    b = LongBatch([left, middle, right])
    rc_, scores, paths = b.run(5.0, 64)
    assert rc_ == _lib.SLK_OK and b.outside_untouched()
    assert scores[1] == -np.inf and (paths[1] == CANARY).all() and len(paths[1]) == 5
    ws = b.ws.cpu().numpy()[PAD:]
    assert (ws[b.ws_off[1]:b.ws_off[1] + b.ws_words[1]] == CANARY).all()
    assert _same(scores[0], paths[0], left) and _same(scores[2], paths[2], right)


# ---- 3: a seeded sweep against the oracle at tile 64 -------------------------------------------------------------------------------------

SWEEP_NEV = (1, 2, 33, 257)


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_equals_oracle_at_tile_64(oracle, seed):
    """Every position count from 3 to 400 times four event counts: one launch per slip penalty, the oracle read by read."""
    need_gpu()
    from sloika_amd import _lib
    reads = []
    for npos in range(3, 401):
        for nev in SWEEP_NEV:
            lt, seq, _ = rc.sweep_read(seed, nev, npos)
            reads.append(dict(ltrans=lt, seq=seq))
    b = LongBatch(reads)
    for slip in (0.0, 2.5, 5.0):
        rc_, scores, paths = b.run(slip, 64)
        assert rc_ == _lib.SLK_OK and b.outside_untouched()

        def want(r):
            return oracle.map_to_sequence(r["ltrans"], r["seq"], slip)
        with ThreadPoolExecutor(8) as pool:
            wanted = list(pool.map(want, reads))
        longest = [int(rc.jumps_of(p).max()) if len(p) > 1 else 0 for _, p in wanted]
        over64, over128 = sum(j >= 64 for j in longest), sum(j >= 128 for j in longest)
        print("seed %d slip %g: %d reads, %d with a jump of 64 or more, %d of 128 or more" % (seed, slip, len(wanted), over64, over128))
        assert over64 >= 200 and over128 >= 80, "the sweep left the regime where tiles of 64 matter"
        bad = [(b.nev[r], b.npos[r]) for r, (s, p) in enumerate(wanted)
               if not (np.array_equal(paths[r], p) and _bits(scores[r]) == _bits(s))]
        assert not bad, (slip, bad[:10])


# ---- 4: the long fixture ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1024, 4096, 0])
def test_long_fixture_through_the_single_entry(tile):
    need_gpu()
    from sloika_amd import _lib
    for name in lc.NAMES:
        c = long_case(name)
        rc_, score, path, untouched, _ = _single_long(c, tile)
        assert rc_ == _lib.SLK_OK and untouched, name
        assert _same(score, path, c), (name, tile, float(score), float(c["score"]), np.flatnonzero(path != c["path"])[:4].tolist())


def _short_between(name, seed, slip, pi, pf, oracle):
    """A short read of the slip fixture for a batch at `slip` with the given priors: its stored answer where the batch runs it as
    the fixture did, the oracle's otherwise."""
    c = dict(slip_case(name))
    if (slip, pi, pf) != (c["slip"], c["pi"] is not None, c["pf"] is not None):
        c["pi"], c["pf"] = rc.priors(seed, len(c["seq"]), pi, pf)
        c["score"], c["path"] = oracle.map_to_sequence(c["ltrans"], c["seq"], slip, prior_initial=c["pi"], prior_final=c["pf"])
    return c


def _long_batches(oracle):
    """The long fixture as batches over the same states, slip and priors, with short reads of the slip fixture between them:
    -> [(slip, has prior_initial, has prior_final, reads)]."""
    def between(slip, pi, pf):
        return _short_between("npos_3", 801, slip, pi, pf, oracle), _short_between("npos_65", 802, slip, pi, pf, oracle)
    out = []
    a, b_ = between(5.0, False, False)
    out.append((5.0, False, False, [long_case("long_5847"), a, long_case("long_8191"), b_, long_case("long_11693"),
                                    long_case("long_16385")]))
    a, b_ = between(5.0, True, True)
    out.append((5.0, True, True, [a, long_case("long_8193"), b_]))
    a, b_ = between(0.0, False, True)
    out.append((0.0, False, True, [b_, long_case("long_8192"), a]))
    a, b_ = between(2.5, False, False)
    out.append((2.5, False, False, [a, long_case("long_8194"), b_]))
    out.append((5.0, False, False, [slip_case("npos_2336"), long_case("long_11693_big"), slip_case("npos_2337")]))
    return out


def test_long_fixture_in_batches_with_short_reads_between(oracle):
    need_gpu()
    from sloika_amd import _lib, transducer
    seen = set()
    for slip, pi, pf, reads in _long_batches(oracle):
        seen.update(c["name"] for c in reads)
        b = LongBatch(reads, pi, pf)
        rc_, scores, paths = b.run(slip, 0)
        assert rc_ == _lib.SLK_OK and b.outside_untouched()
        for c, s, p in zip(reads, scores, paths):
            assert _same(s, p, c), c["name"]
        scores, paths = transducer.map_to_sequence_batch([c["ltrans"] for c in reads], [c["seq"] for c in reads], slip,
                                                         prior_initial=[c["pi"] for c in reads] if pi else None,
                                                         prior_final=[c["pf"] for c in reads] if pf else None, long_reference=True)
        for c, s, p in zip(reads, scores, paths):
            assert _same(s, p, c), c["name"]
    assert seen >= set(lc.NAMES) | {"npos_3", "npos_65"}


@pytest.mark.parametrize("name", lc.NAMES)
def test_long_fixture_through_map_to_sequence(name):
    need_gpu()
    from sloika_amd import _lib, transducer
    c = long_case(name)
    score, path = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=c["slip"], prior_initial=c["pi"], prior_final=c["pf"],
                                             long_reference=True)
    assert _same(score, path, c), name
    with pytest.raises(_lib.SloikaAmdError):                       # without the keyword the refusal stands
        transducer.map_to_sequence(c["ltrans"][:2], c["seq"], slip=c["slip"])


def test_a_call_whose_reads_all_fit_is_unchanged_by_the_keyword():
    need_gpu()
    from sloika_amd import transducer
    cases = [slip_case("npos_2337"), slip_case("npos_5846"), slip_case("npos_2336")]
    scores, paths = transducer.map_to_sequence_batch([c["ltrans"] for c in cases], [c["seq"] for c in cases], 5.0, long_reference=True)
    for c, s, p in zip(cases, scores, paths):
        assert _same(s, p, c), c["name"]
        s1, p1 = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=5.0, long_reference=True)
        assert _same(s1, p1, c), c["name"]


# ---- 5: the default tile's own edges ----------------------------------------------------------------------------------------------------

def test_default_tile_edges_equal_oracle(oracle):
    need_gpu()
    from sloika_amd import _lib, transducer
    D = transducer.DEFAULT_TILE
    reads = []
    for i, npos in enumerate((D - 1, D, D + 1, D + 2, D + 3, 2 * D + 1, 2 * D + 2)):
        # one jump from in front of the first tile edge to behind the last one, and a short one
        # (1025 states: with 65 a read would rather hop between matching k-mers, 64 positions apart, than jump this far)
        lt, seq, _ = rc.planted(9100 + i, 40, npos, 1025, jumps=[(12, npos - 40), (30, 7)], start=3, contrast=8.0 * npos)
        c = dict(name="edge_%d" % npos, ltrans=lt, seq=seq, pi=None, pf=None, slip=5.0)
        c["score"], c["path"] = oracle.map_to_sequence(lt, seq, 5.0)
        assert (rc.jumps_of(c["path"]) >= npos - 40).any(), "the read no longer jumps across the tile edges"
        reads.append(c)
    for tile in (0, D):
        b = LongBatch(reads)
        rc_, scores, paths = b.run(5.0, tile)
        assert rc_ == _lib.SLK_OK and b.outside_untouched()
        for c, s, p in zip(reads, scores, paths):
            assert _same(s, p, c), (tile, c["name"])
    for c in reads:
        rc_, score, path, untouched, _ = _single_long(c, 0)
        assert rc_ == _lib.SLK_OK and untouched and _same(score, path, c), c["name"]


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------

def test_bad_tiles_and_a_short_workspace_are_refused_before_anything_is_written():
    need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    c = slip_case("npos_195")
    for tile in (32, 96, -64, 6784 + 64):
        assert L.slk_map_to_sequence_long_workspace_bytes(40, 195, tile) == 0
        rc_, _, _, untouched, nothing = _single_long(c, tile)
        assert rc_ == _lib.SLK_ERR_INVALID_ARG and untouched and nothing, tile
        b = LongBatch([slip_case("npos_65"), c])
        assert b.run(5.0, tile)[0] == _lib.SLK_ERR_INVALID_ARG and b.outside_untouched() and b.nothing_written(), tile
    rc_, _, _, untouched, nothing = _single_long(c, 64, short_by=1)
    assert rc_ == _lib.SLK_ERR_WORKSPACE and untouched and nothing
    rc_, score, path, untouched, _ = _single_long(c, 64)
    assert rc_ == _lib.SLK_OK and untouched and _same(score, path, c)


# ---- 7: workspace_limit -----------------------------------------------------------------------------------------------------------------

def test_workspace_limit_splits_the_batch_and_changes_nothing():
    need_gpu()
    from sloika_amd import transducer
    cases = [long_case(n) for n in ("long_5847", "long_8191", "long_8193", "long_11693", "long_16385")]      # all at slip 5, no priors
    lts, seqs = [c["ltrans"] for c in cases], [c["seq"] for c in cases]
    nbytes = [4 * _ws_words(len(lt), len(q)) for lt, q in zip(lts, seqs)]
    whole = transducer.map_to_sequence_batch(lts, seqs, 5.0, long_reference=True)
    for limit, least in ((20 << 20, 3), (max(nbytes) - 1, 3)):
        runs = transducer.workspace_runs(nbytes, limit)
        assert len(runs) >= least and runs[0][0] == 0 and runs[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert all(sum(nbytes[lo:hi]) <= limit or hi - lo == 1 for lo, hi in runs)
        scores, paths = transducer.map_to_sequence_batch(lts, seqs, 5.0, long_reference=True, workspace_limit=limit)
        assert np.array_equal(_bits(scores), _bits(whole[0])) and all(np.array_equal(p, q) for p, q in zip(paths, whole[1]))
    assert max(nbytes) > 15 << 20                                  # the second limit is below the largest read: it still ran
    for c, lt, q, s, p in zip(cases, lts, seqs, *whole):
        s1, p1 = transducer.map_to_sequence(lt, q, slip=5.0, long_reference=True)
        assert _bits(s1) == _bits(s) and np.array_equal(p1, p)
        if c["pi"] is None and c["pf"] is None:
            assert _same(s, p, c), c["name"]


# ---- 8: repeatability (a screen for hazards in the double buffer of score rows; run as written) ---------------------------------------------

def test_repeated_launches_give_identical_bits():
    need_gpu()
    from sloika_amd import _lib
    c = long_case("long_11693_big")
    first = _single_long(c, 0)
    assert first[0] == _lib.SLK_OK and _same(first[1], first[2], c)
    for _ in range(2):
        again = _single_long(c, 0)
        assert again[0] == _lib.SLK_OK and _bits(again[1]) == _bits(first[1]) and np.array_equal(again[2], first[2])


# ---- 9, 10: end to end ------------------------------------------------------------------------------------------------------------------

def late_read(seed=78, nbase=5900, nstep=320, skip=100, start=5200, stride=5):
    """rc.skipping_read on a reference of more than 5851 bases, the read starting `start` positions into it: -> (reference bytes,
    signal float32 [nstep * stride], posterior float32 [nstep, 1025])."""
    rs = np.random.RandomState(seed)
    ref = bytes(rs.choice(list(b"ACGT"), size=nbase).tolist())
    digits = np.asarray([b"ACGT".index(c) for c in ref], dtype=np.int64)
    npos = nbase - 4
    states = 1 + sum(digits[j:j + npos] * 4 ** (4 - j) for j in range(5))
    path = rc.plant_path(rs, nstep, npos, [(nstep // 2, skip)], start=start)
    moved = np.ones(nstep, dtype=bool)
    moved[1:] = np.diff(path) != 0
    post = np.full((nstep, 1025), 0.1 / 1024, dtype=np.float32)
    post[np.arange(nstep), np.where(moved, states[path], 0)] = np.float32(0.9)
    signal = (90.0 + 12.0 * rs.random_sample(nstep * stride)).astype(np.float32)
    return ref, signal, post


def _same_raw(got, want, ref, signal):
    from sloika_amd import chunkify_raw as cr
    score, table, path, seq = got
    want_score, want_cols, want_path, want_seq = want
    assert _bits(score) == _bits(want_score)
    assert path.dtype == np.int64 and np.array_equal(path, want_path) and list(seq) == list(want_seq)
    for f in ("start", "length", "seq_pos", "move"):
        assert table[f].dtype == np.int64 and np.array_equal(table[f], want_cols[f]), f
    kmers = np.array([ref[i:i + 5] for i in range(len(ref) - 4)])
    assert np.array_equal(table["kmer"], kmers[want_cols["seq_pos"]]) and table["good_emission"].all()
    assert cr.mapping_table_is_registered(signal, table)


def test_raw_remap_of_a_read_on_a_long_reference():
    need_gpu()
    import torch
    from sloika_amd import _lib, batch, chunkify_raw as cr
    batch.init_chunk_identity_worker(5, b"ACGT")
    long_ = late_read()
    short = rc.skipping_read()
    posts = {len(r[1]): r[2] for r in (long_, short)}
    assert len(posts) == 2 and len(long_[0]) > 5851

    def calc_post(inmat):
        assert inmat.shape[1:] == (1, 1)
        return torch.from_numpy(posts[inmat.shape[0]][:, None, :]).to(inmat.device)
    prior, slip = (25.0, 25.0), 5.0
    want = [oracle_remap.raw_remap(ref, signal, post, 1e-5, 5, prior, slip) for ref, signal, post in (long_, short)]
    assert want[0][2].min() > 5000 and (np.diff(want[0][2]) >= 90).any(), "the long read no longer skips late in its reference"
    _same_raw(cr.raw_remap(long_[0], long_[1], 1e-5, 5, prior, slip, calc_post=calc_post, long_reference=True), want[0], *long_[:2])
    many = cr.raw_remap_many([long_[0], short[0]], [long_[1], short[1]], 1e-5, 5, prior, slip, calc_post=calc_post,
                             long_reference=True)
    assert len(many) == 2
    _same_raw(many[0], want[0], *long_[:2])
    _same_raw(many[1], want[1], *short[:2])
    with pytest.raises(_lib.SloikaAmdError):
        cr.raw_remap(long_[0], long_[1], 1e-5, 5, prior, slip, calc_post=calc_post)


def test_event_remap_many_with_a_long_reference(tiny_gru, worker_state):           # noqa: F811
    batch = worker_state
    from tests.event_remap_ref import erc
    batch.init_chunk_identity_worker(5, erc.ALPHABET)
    refs, evs = random_reads()
    refs = [refs[0], refs[1], (b"ACGT" * 1463)[:5851]]               # 5847 positions: one more than the LDS-resident kernel takes
    calc_post = tiny_gru.compile()
    prior, slip = (25.0, 25.0), 5.0
    many = batch.remap_many(refs, evs, 1e-5, 5, prior, slip, network=tiny_gru, long_reference=True)
    assert len(many) == 3
    for ref, ev, (score, table, path, seq) in zip(refs, evs, many):
        s1, t1, p1, q1 = batch.remap(ref, ev, 1e-5, 5, prior, slip, calc_post=calc_post, long_reference=True)
        assert np.isfinite(score) and _bits(score) == _bits(s1), (score, s1)
        assert np.array_equal(path, p1) and path.dtype == p1.dtype and len(path) == len(ev)
        assert list(seq) == list(q1) and len(seq) == len(ref) - 4
        assert table.dtype == t1.dtype and np.array_equal(table, t1)
    plain = batch.remap_many(refs[:2], evs[:2], 1e-5, 5, prior, slip, network=tiny_gru)
    for (sa, ta, pa, _), (sb, tb, pb, _) in zip(many, plain):
        assert _bits(sa) == _bits(sb) and np.array_equal(pa, pb) and np.array_equal(ta, tb)
