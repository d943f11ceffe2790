"""The remap DP (csrc/transducer.hip) where reads slip: long jumps, the edges of the backtrace's window and batches, the padded
in-LDS slip scan at its segment boundaries, the LDS request above 64 KB and its limit, the empty-read branch of the batch kernel
and the arg-max with distant ties.  Bit for bit against what the REFERENCE returned (tests/golden/remap_slips.npz; the
conditions that keep that fixture in the long-slip regime are checked without a GPU in tests/test_oracle_remap_slips.py), and,
on a seeded sweep, against the oracle that the same fixture pins."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle_remap
from tests.gpu_util import need_gpu
from tests.test_oracle_remap_slips import rc, slip_case

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
PAD = 256                                   # canary words on either side of an output
SCORE_CANARY = np.float32(-12345.5)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _same(score, path, c):
    return np.array_equal(path, c["path"]) and path.dtype == np.int32 and _bits(score) == _bits(c["score"])


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, offset_words=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_words)


def _canary(n):
    import torch
    return torch.full((n + 2 * PAD,), CANARY, dtype=torch.int32, device="cuda")


def _outside_untouched(buf, n):
    """The canary words round the `n` words that a call may write."""
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all())


class Batch(object):
    """Reads laid out for slk_map_to_sequence_batch_f32, uploaded once; the outputs sit inside canaries."""

    def __init__(self, reads, priors=False):
        import torch
        self.nev = [len(r["ltrans"]) for r in reads]
        self.npos = [len(r["seq"]) for r in reads]
        self.nst = reads[0]["ltrans"].shape[1]
        self.ev_off = np.concatenate([[0], np.cumsum(self.nev)]).astype(np.int64)
        pos_off = np.concatenate([[0], np.cumsum(self.npos)]).astype(np.int64)
        ws = np.asarray([e * p for e, p in zip(self.nev, self.npos)], dtype=np.int64)
        ws_off = np.concatenate([[0], np.cumsum(ws)[:-1]]).astype(np.int64)
        self.nws = int(ws.sum())
        self.lt = _dev(np.concatenate([r["ltrans"].reshape(-1, self.nst) for r in reads]))
        self.seq = _dev(np.concatenate([r["seq"] for r in reads]).astype(np.int32))
        self.pi = _dev(np.concatenate([r["pi"] for r in reads])) if priors else None
        self.pf = _dev(np.concatenate([r["pf"] for r in reads])) if priors else None
        self.off = [_dev(a) for a in (self.ev_off, pos_off, ws_off)]
        self.torch = torch

    def run(self, slip, max_npos=None):
        from sloika_amd import _lib, device as D
        torch = self.torch
        nread = len(self.nev)
        self.ws = _canary(self.nws)
        self.path = _canary(int(self.ev_off[-1]))
        self.score = torch.full((nread,), float(SCORE_CANARY), dtype=torch.float32, device="cuda")
        rc_ = _lib.lib().slk_map_to_sequence_batch_f32(
            _ptr(self.lt), self.nst, _ptr(self.off[0]), _ptr(self.seq), _ptr(self.off[1]), nread,
            max(self.npos) if max_npos is None else max_npos, float(slip), _ptr(self.pi), _ptr(self.pf), _ptr(self.ws, PAD),
            _ptr(self.off[2]), _ptr(self.score), _ptr(self.path, PAD), D.stream_ptr())
        torch.cuda.synchronize()
        ph = self.path.cpu().numpy()[PAD:]
        return rc_, self.score.cpu().numpy(), [ph[self.ev_off[b]:self.ev_off[b + 1]] for b in range(nread)]

    def outside_untouched(self):
        return _outside_untouched(self.path, int(self.ev_off[-1])) and _outside_untouched(self.ws, self.nws)


def _single_abi(c, nev=None, npos=None):
    """slk_map_to_sequence_f32 with path_out and the workspace inside canaries -> (rc, score, path, untouched outside)."""
    import torch
    from sloika_amd import _lib, device as D
    nev = len(c["ltrans"]) if nev is None else nev
    npos = len(c["seq"]) if npos is None else npos
    lt, seq, pi, pf = _dev(c["ltrans"]), _dev(c["seq"]), _dev(c["pi"]), _dev(c["pf"])
    ws, path = _canary(nev * npos), _canary(nev)
    score = torch.full((1,), float(SCORE_CANARY), dtype=torch.float32, device="cuda")
    rc_ = _lib.lib().slk_map_to_sequence_f32(_ptr(lt), nev, c["ltrans"].shape[1], _ptr(seq), npos, float(c["slip"]), _ptr(pi),
                                             _ptr(pf), _ptr(ws, PAD), 4 * nev * npos, _ptr(score), _ptr(path, PAD),
                                             D.stream_ptr())
    torch.cuda.synchronize()
    untouched = _outside_untouched(path, nev) and _outside_untouched(ws, nev * npos)
    return rc_, np.float32(score.item()), path.cpu().numpy()[PAD:PAD + nev], untouched


# ---- single reads ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.NAMES)
def test_single_read_equals_reference(name):
    need_gpu()
    from sloika_amd import transducer
    c = slip_case(name)
    score, path = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=c["slip"], prior_initial=c["pi"], prior_final=c["pf"])
    assert _same(score, path, c), (name, float(score), c["score"], np.flatnonzero(path != c["path"])[:8])


@pytest.mark.parametrize("name", rc.NAMES)
def test_single_read_through_the_c_abi_writes_its_outputs_only(name):
    need_gpu()
    from sloika_amd import _lib
    c = slip_case(name)
    rc_, score, path, untouched = _single_abi(c)
    assert rc_ == _lib.SLK_OK and _same(score, path, c), name
    assert untouched, "words outside path_out[0, nev) or the nev * npos words of the workspace changed"


# ---- batches -----------------------------------------------------------------------------------------------------------------------

def _big_next_to_small(cases):
    """Largest, smallest, second largest, second smallest, ..."""
    order = sorted(cases, key=lambda c: len(c["ltrans"]) * len(c["seq"]))
    out = []
    while order:
        out.append(order.pop())
        if order:
            out.append(order.pop(0))
    return out


def _plain(name):
    c = rc.CASES[name]
    return c["pri"] == (False, False) and c["tie_gap"] is None


_GROUPS = sorted({(rc.CASES[n]["gen"]["nst"], rc.CASES[n]["slip"]) for n in rc.NAMES if _plain(n)})


@pytest.mark.parametrize("nst,slip", _GROUPS)
def test_batch_equals_reference_and_single_calls(nst, slip):
    """All cases over the same states and slip in ONE launch, through the Python wrapper and through the C ABI with canaries."""
    need_gpu()
    from sloika_amd import _lib, transducer
    cases = _big_next_to_small([slip_case(n) for n in rc.NAMES
                                if _plain(n) and (rc.CASES[n]["gen"]["nst"], rc.CASES[n]["slip"]) == (nst, slip)])
    scores, paths = transducer.map_to_sequence_batch([c["ltrans"] for c in cases], [c["seq"] for c in cases], slip)
    b = Batch(cases)
    rc_, scores2, paths2 = b.run(slip)
    assert rc_ == _lib.SLK_OK and b.outside_untouched()
    for c, s, p, s2, p2 in zip(cases, scores, paths, scores2, paths2):
        assert _same(s, p, c) and _same(s2, p2, c), c["name"]
        s1, p1 = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=slip)
        assert _same(s1, p1, c), c["name"]


def test_batch_with_priors_on_every_read(oracle):
    need_gpu()
    from sloika_amd import transducer
    reads = []
    for i, name in enumerate(["prior_both", "jumps_n65_s5", "npos_3", "bt_first", "npos_195", "nev_1", "bt_consecutive",
                              "edge_small", "nev_65", "npos_131"]):
        c = dict(slip_case(name))
        if name != "prior_both":                                 # the fixture's own read keeps its priors and its stored answer
            c["pi"], c["pf"] = rc.priors(900 + i, len(c["seq"]), True, True)
            c["score"], c["path"] = oracle.map_to_sequence(c["ltrans"], c["seq"], 5.0, prior_initial=c["pi"], prior_final=c["pf"])
        reads.append(c)
    assert any((rc.jumps_of(c["path"]) >= rc.WINDOW).any() for c in reads[1:])
    scores, paths = transducer.map_to_sequence_batch([c["ltrans"] for c in reads], [c["seq"] for c in reads], 5.0,
                                                     prior_initial=[c["pi"] for c in reads], prior_final=[c["pf"] for c in reads])
    for c, s, p in zip(reads, scores, paths):
        assert _same(s, p, c), c["name"]
        s1, p1 = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=5.0, prior_initial=c["pi"], prior_final=c["pf"])
        assert _same(s1, p1, c), c["name"]


# ---- seeded sweep against the oracle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sweep_equals_oracle(oracle, seed):
    """Every position count from 3 to 400 and five large ones, times five event counts, times three slip penalties: one launch
    per slip, the oracle read by read."""
    need_gpu()
    from sloika_amd import _lib
    reads = []
    for npos in rc.SWEEP_NPOS:
        for nev in rc.SWEEP_NEV:
            lt, seq, _ = rc.sweep_read(seed, nev, npos)
            reads.append(dict(ltrans=lt, seq=seq))
    b = Batch(reads)
    for slip in rc.SWEEP_SLIP:
        rc_, scores, paths = b.run(slip)
        assert rc_ == _lib.SLK_OK and b.outside_untouched()

        def want(r):
            return oracle.map_to_sequence(r["ltrans"], r["seq"], slip)
        with ThreadPoolExecutor(8) as pool:
            wanted = list(pool.map(want, reads))
        long_jumps = sum(bool((rc.jumps_of(p) >= rc.WINDOW).any()) for _, p in wanted)
        print("seed %d slip %g: %d reads, %d with a jump of 64 or more" % (seed, slip, len(wanted), long_jumps))
        assert long_jumps >= 100, "the sweep left the long-slip regime"
        bad = [(b.nev[r], b.npos[r]) for r, (s, p) in enumerate(wanted)
               if not (np.array_equal(paths[r], p) and _bits(scores[r]) == _bits(s))]
        assert not bad, (slip, bad[:10])


# ---- limits -----------------------------------------------------------------------------------------------------------------------

def test_limits_5846_positions_run_5847_are_refused():
    need_gpu()
    from sloika_amd import _lib, transducer
    c = slip_case("npos_5846")
    small = slip_case("npos_3")
    b = Batch([slip_case("npos_2337"), c, slip_case("npos_2336")])
    rc_, scores, paths = b.run(5.0)
    assert rc_ == _lib.SLK_OK and _same(scores[1], paths[1], c) and b.outside_untouched()
    assert _same(scores[0], paths[0], slip_case("npos_2337")) and _same(scores[2], paths[2], slip_case("npos_2336"))
    # one position more than fits: refused by both entry points before anything is written
    rs = np.random.RandomState(5)
    over = dict(ltrans=c["ltrans"][:2], seq=rs.randint(1, 1025, size=5847).astype(np.int32), pi=None, pf=None, slip=5.0)
    rc_, score, path, untouched = _single_abi(over)
    assert rc_ == _lib.SLK_ERR_UNSUPPORTED and untouched and (path == CANARY).all() and score == SCORE_CANARY
    b = Batch([slip_case("npos_2337"), over])
    rc_, scores, paths = b.run(5.0)
    assert rc_ == _lib.SLK_ERR_UNSUPPORTED and b.outside_untouched()
    assert all((p == CANARY).all() for p in paths) and (scores == SCORE_CANARY).all() and (b.ws.cpu().numpy() == CANARY).all()
    # the same from a caller that claims 5847 for reads that are all shorter
    b = Batch([small, slip_case("npos_65")])
    rc_, scores, paths = b.run(5.0, max_npos=5847)
    assert rc_ == _lib.SLK_ERR_UNSUPPORTED and b.outside_untouched()
    assert all((p == CANARY).all() for p in paths) and (scores == SCORE_CANARY).all() and (b.ws.cpu().numpy() == CANARY).all()
    assert b.run(5.0, max_npos=5846)[0] == _lib.SLK_OK
    with pytest.raises(_lib.SloikaAmdError):
        transducer.map_to_sequence(over["ltrans"], over["seq"], slip=5.0)
    with pytest.raises(_lib.SloikaAmdError):
        transducer.map_to_sequence_batch([c["ltrans"], over["ltrans"]], [c["seq"], over["seq"]], 5.0)


# ---- empty reads (reachable through the C ABI only: the Python wrapper refuses them) ---------------------------------------------------

@pytest.mark.parametrize("empty", ["no_events", "two_positions"])
def test_empty_read_in_the_middle_of_a_batch(empty):
    need_gpu()
    from sloika_amd import _lib
    left, right = slip_case("bt_last"), slip_case("nev_33")
    if empty == "no_events":
        middle = dict(ltrans=np.zeros((0, 65), dtype=np.float32), seq=left["seq"][:7])
    else:
        middle = dict(ltrans=right["ltrans"][:5], seq=left["seq"][:2])
    b = Batch([left, middle, right])
    rc_, scores, paths = b.run(5.0)
    assert rc_ == _lib.SLK_OK and b.outside_untouched()
    assert scores[1] == -np.inf and (paths[1] == CANARY).all() and len(paths[1]) == len(middle["ltrans"])
    assert _same(scores[0], paths[0], left) and _same(scores[2], paths[2], right)
    for c, s, p in ((left, scores[0], paths[0]), (right, scores[2], paths[2])):
        rc1, s1, p1, _ = _single_abi(c)
        assert rc1 == _lib.SLK_OK and np.array_equal(p1, p) and _bits(s1) == _bits(s)
    ws = b.ws.cpu().numpy()[PAD:]
    lo = len(left["ltrans"]) * len(left["seq"])
    assert (ws[lo:lo + len(middle["ltrans"]) * len(middle["seq"])] == CANARY).all(), "the empty read's workspace was written"


# ---- repeatability (a screen for hazards in the LDS double buffers; run as written) ----------------------------------------------------

def test_repeated_launches_give_identical_bits():
    need_gpu()
    from sloika_amd import _lib
    c = slip_case("npos_5846")
    first = _single_abi(c)
    assert first[0] == _lib.SLK_OK and _same(first[1], first[2], c)
    for _ in range(2):
        again = _single_abi(c)
        assert again[0] == _lib.SLK_OK and _bits(again[1]) == _bits(first[1]) and np.array_equal(again[2], first[2])
    reads = []
    for i in range(64):
        lt, seq, _ = rc.sweep_read(9, 257, 70 + 37 * i)
        reads.append(dict(ltrans=lt, seq=seq))
    b = Batch(reads)
    rc_, scores, paths = b.run(2.5)
    assert rc_ == _lib.SLK_OK and np.isfinite(scores).all()
    for _ in range(2):
        rc2, scores2, paths2 = b.run(2.5)
        assert rc2 == _lib.SLK_OK and np.array_equal(_bits(scores2), _bits(scores))
        assert all(np.array_equal(p, q) for p, q in zip(paths, paths2))


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_raw_remap_of_a_read_that_skips_a_hundred_bases():
    need_gpu()
    import torch
    from sloika_amd import batch, chunkify_raw as cr
    batch.init_chunk_identity_worker(5, b"ACGT")
    ref, signal, post = rc.skipping_read()

    def calc_post(inmat):
        assert inmat.shape[1:] == (1, 1)
        return torch.from_numpy(post[:, None, :]).to(inmat.device)
    prior, slip = (25.0, 25.0), 5.0
    want_score, want_cols, want_path, want_seq = oracle_remap.raw_remap(ref, signal, post, 1e-5, 5, prior, slip)
    assert (np.diff(want_path) >= 90).any(), "the read no longer skips"
    score, table, path, seq = cr.raw_remap(ref, signal, 1e-5, 5, prior, slip, calc_post=calc_post)
    assert _bits(score) == _bits(want_score)
    assert path.dtype == np.int64 and np.array_equal(path, want_path) and list(seq) == list(want_seq)
    for f in ("start", "length", "seq_pos", "move"):
        assert table[f].dtype == np.int64 and np.array_equal(table[f], want_cols[f]), f
    kmers = np.array([ref[i:i + 5] for i in range(len(ref) - 4)])
    assert np.array_equal(table["kmer"], kmers[want_cols["seq_pos"]]) and table["good_emission"].all()
    assert cr.mapping_table_is_registered(signal, table)
