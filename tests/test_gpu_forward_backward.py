"""Forward-backward on the device (csrc/forward_backward.hip through decode.forwards_backwards / forwards_backwards_batch and
pipeline.Basecaller.occupancy_chunks; design/forward_backward.md).

The truth is tests/forward_backward_ref.py in np.longdouble.  The yardstick is E_occ, the largest distance of the same oracle in
float64 from that truth over the cases below, computed here on the CPU; the float64 entry may be 4 E_occ + 2^-60 (L + 1) away from
the truth (the allowance design/forward_score.md 5 gives a float64 device result, plus the fixed-point quantum of each term).
Measured on an MI355X: E_occ 6.0e-16, the largest |occ - truth| 0.36 E_occ.  Everything else is bit equality or exact structure."""
import ctypes
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.gpu_util import need_gpu, dev, stream

sys.path.insert(0, GOLDEN)
import forward_cases as fc                               # noqa: E402

from tests import forward_backward_ref as fbr            # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
ALLOW = 4.0
QUANTUM = 2.0 ** -60
SENTINEL = -7.25
STATES = (1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 2049)

# name -> (T, S, L, kind of sequence, modes); blank = the last column unless the kind says otherwise
CASES = {
    "small": (40, 5, 12, "random", (False, True)),
    "long_full": (300, 5, 120, "random", (True,)),
    "mid": (150, 65, 60, "random", (False, True)),
    "wide": (64, 1025, 30, "random", (False, True)),
    "short_free": (8, 5, 700, "random", (False,)),           # four states per thread
    "short_long": (8, 5, 5000, "random", (False,)),          # 32 states per thread: the largest register budget
    "repeat": (40, 5, 17, "repeat", (False, True)),          # every position carries the same symbol: one slot takes every term
    "blank_symbol": (40, 5, 14, "blank", (False, True)),     # some positions carry the blank's own column
}


def build(name, dtype="float64"):
    T, S, L, kind, _ = CASES[name]
    seed = 5000 + sorted(CASES).index(name)
    post = fc.make_post(seed, T, S, dtype)
    seq = fc.make_seq(seed, S, L, "random" if kind == "blank" else kind)
    if kind == "blank":
        seq[::4] = S - 1
    return post, seq


def entries():
    return [(n, full) for n in CASES for full in CASES[n][4]]


@pytest.fixture(scope="module")
def oracle():
    """Per entry the truth (np.longdouble) and the float64 oracle, once; E_occ is the float64 oracle's largest distance from the truth."""
    out, e_occ = {}, 0.0
    for name, full in entries():
        post, seq = build(name)
        truth = fbr.forwards_backwards(post, seq, full=full, dtype=LD, gaps=True)
        mine = fbr.forwards_backwards(post, seq, full=full)
        e_occ = max(e_occ, float(np.abs(mine[1] - truth[1]).max()), float(np.abs(mine[3] - truth[3]).max()))
        out[name, full] = truth
    assert 0.0 < e_occ < 1e-13                            # a float64 recursion's distance from the exact value, not a tolerance
    out["E_occ"] = e_occ
    return out


def bound(oracle, L):
    return ALLOW * oracle["E_occ"] + QUANTUM * (L + 1)


def host(r):
    score, occ, row, prob = r
    return (score.cpu().numpy(), None if occ is None else occ.cpu().numpy(), None if row is None else [v.cpu().numpy() for v in row],
            None if prob is None else [v.cpu().numpy() for v in prob])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def packed(pairs):
    rows = np.concatenate([p for p, _ in pairs])
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p, _ in pairs])]).astype(np.int64)
    return rows, off


def run_packed(pairs, **kw):
    """-> per pair (score, occ rows, emit_row, emit_prob) as numpy."""
    from sloika_amd import decode
    rows, off = packed(pairs)
    score, occ, row, prob = host(decode.forwards_backwards_batch(dev(rows), [s for _, s in pairs], row_off=off, **kw))
    return [(score[b], occ[off[b]:off[b + 1]], row[b], prob[b]) for b in range(len(pairs))]


def same_results(a, b):
    return all(same(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


# ---- 1: the score has the forward score's bits ------------------------------------------------------------------------------------

@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("variant", ["float32", "float32_min_prob", "float64"])
def test_score_bits(full, variant):
    """L + 1 at every ownership boundary: free on 6 rows; full on 300 rows up to 257 states, on 6 rows (-inf) beyond."""
    need_gpu()
    from sloika_amd import decode
    dtype = "float64" if variant == "float64" else "float32"
    mp = 1e-5 if variant == "float32_min_prob" else None
    pairs = []
    for n in STATES:
        T = 300 if full and n <= 257 else 6
        pairs.append((fc.make_post(6000 + n, T, 5, dtype), fc.make_seq(6000 + n, 5, n - 1, "random")))
    rows, off = packed(pairs)
    rows_d, seqs = dev(rows), [s for _, s in pairs]
    want = decode.forwards_batch(rows_d, seqs, full=full, row_off=off, min_prob=mp).cpu().numpy()
    got = decode.forwards_backwards_batch(rows_d, seqs, full=full, row_off=off, min_prob=mp)[0].cpu().numpy()
    assert got.dtype == np.float64 and same(got, want), (got, want)
    assert np.isfinite(got[:5]).all()
    if not full:
        assert np.isfinite(got).all()


# ---- 2: accuracy of the float64 entry, row sums, positions ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device64():
    need_gpu()
    out = {}
    for full in (False, True):
        names = [n for n in CASES if full in CASES[n][4]]
        for S in sorted({CASES[n][1] for n in names}):
            group = [n for n in names if CASES[n][1] == S]
            for n, r in zip(group, run_packed([build(n) for n in group], full=full)):
                out[n, full] = r
    return out


def test_accuracy_float64(oracle, device64):
    worst = 0.0
    for name, full in entries():
        L = CASES[name][2]
        score, occ, row, prob = device64[name, full]
        t_score, t_occ, t_row, t_prob, _ = oracle[name, full]
        assert occ.dtype == np.float64 and np.isfinite(score)
        d = max(float(np.abs(occ - t_occ).max()), float(np.abs(prob - t_prob).max()))
        ratio = (d - QUANTUM * (L + 1)) / oracle["E_occ"]
        print("%-14s full=%d  |occ - truth| %.3e  (%.3f E_occ after the quantum; E_occ %.3e)" % (name, full, d, max(ratio, 0.0), oracle["E_occ"]))
        worst = max(worst, d / oracle["E_occ"])
        assert d <= bound(oracle, L), (name, full, d, bound(oracle, L))
        assert abs(score - float(t_score)) <= 1e-12 * max(1.0, abs(float(t_score)))
    print("largest |occ - truth| / E_occ: %.3f" % worst)


def test_row_sums(oracle, device64):
    for name, full in entries():
        score, occ = device64[name, full][:2]
        assert np.isfinite(score)
        assert float(np.abs(occ.sum(axis=1) - 1.0).max()) <= bound(oracle, CASES[name][2]), (name, full)
        assert (occ >= 0).all()


def test_positions(oracle, device64):
    for name, full in entries():
        L = CASES[name][2]
        _, _, row, prob = device64[name, full]
        _, _, t_row, t_prob, gap = oracle[name, full]
        firm = np.asarray(gap > 1e-9)
        assert firm.all(), (name, full, float(gap.min()))          # checked on the CPU: these inputs exclude no position
        assert firm.mean() >= 0.95
        assert row.dtype == np.int32 and np.array_equal(row[firm], t_row[firm]), (name, full)
        assert float(np.abs(prob - t_prob).max()) <= bound(oracle, L)


def test_a_tie_goes_to_the_lowest_row():
    """Two identical consecutive rows, free mode: the move of the one position is as probable in either."""
    need_gpu()
    from sloika_amd import decode
    tie = np.repeat(np.array([[0.125, 0.5, 0.125, 0.125, 0.125]]), 2, axis=0)
    for post in (tie, tie.astype(np.float32)):
        score, occ, row, prob = decode.forwards_backwards(post, [1])
        assert row.tolist() == [0] and occ[0, 1] == occ[1, 1] == post.dtype.type(prob[0]) and occ.dtype == post.dtype


# ---- 3: the float32 entry ---------------------------------------------------------------------------------------------------------

def test_float32_is_float64_rounded_once():
    need_gpu()
    for full in (False, True):
        names = [n for n in ("small", "repeat", "blank_symbol") if full in CASES[n][4]]
        pairs32 = [build(n, "float32") for n in names]
        r32 = run_packed(pairs32, full=full)
        r64 = run_packed([(p.astype(np.float64), s) for p, s in pairs32], full=full)
        for a, b in zip(r32, r64):
            assert a[1].dtype == np.float32 and same(a[1], b[1].astype(np.float32))
            assert same(a[0], b[0]) and same(a[2], b[2]) and same(a[3], b[3])


def test_float32_with_min_prob(oracle):
    """The occupancies refer to decode.prepare_post's float32 values: the oracle is fed those."""
    need_gpu()
    mp = 1e-5
    for name in ("small", "mid", "wide"):
        post, seq = build(name, "float32")
        prepared = (np.float32(mp) + np.float32(1.0 - mp) * post).astype(np.float32)         # decode.py:36 in float32
        for full in (False, True):
            (score, occ, row, prob), = run_packed([(post, seq)], full=full, min_prob=mp)
            t = fbr.forwards_backwards(prepared, seq, full=full, dtype=LD)
            tol = bound(oracle, len(seq)) + 2.0 ** -24
            assert float(np.abs(occ - t[1]).max()) <= tol and float(np.abs(prob - t[3]).max()) <= bound(oracle, len(seq))
            assert np.array_equal(row, t[2])
            (_, occ_p, row_p, prob_p), = run_packed([(prepared, seq)], full=full)
            assert same(occ, occ_p) and same(row, row_p) and same(prob, prob_p)             # the transform inside is prepare_post's


# ---- 4: the same bits everywhere --------------------------------------------------------------------------------------------------

def ragged_pairs():
    """Seven float32 pairs over 65 states: one row, no positions, a wave's and the workgroup's edge, two and four states per thread."""
    shapes = [(1, 1), (40, 0), (300, 254), (280, 256), (200, 64), (77, 30), (8, 700)]
    return [(fc.make_post(7000 + i, T, 65, "float32"), fc.make_seq(7000 + i, 65, L, "random")) for i, (T, L) in enumerate(shapes)]


def network_layout(pairs, pad=0):
    S = pairs[0][0].shape[1]
    tmax = max(p.shape[0] for p, _ in pairs)
    x = np.full((tmax, len(pairs), S + pad), np.float32(np.nan), dtype=np.float32)
    for b, (p, _) in enumerate(pairs):
        x[:p.shape[0], b, :S] = p
    return x, np.array([p.shape[0] for p, _ in pairs], dtype=np.int32)


@pytest.mark.parametrize("full", [False, True])
def test_same_bits_in_any_batch_layout_and_launch(full):
    need_gpu()
    from sloika_amd import decode, transducer, _lib
    pairs = ragged_pairs()
    seqs = [s for _, s in pairs]
    B = len(pairs)
    batch = run_packed(pairs, full=full)
    assert np.isfinite([r[0] for r in batch]).all() or full
    for b in range(B):                                                                     # alone
        (alone,) = run_packed([pairs[b]], full=full)
        assert same_results(alone, batch[b]), b
    again = run_packed(pairs, full=full)                                                   # a second launch
    assert all(same_results(x, y) for x, y in zip(again, batch))
    for pad in (0, 3):                                                                     # the network layout, ld and occ_ld at 65 and at 68
        net, lens = network_layout(pairs, pad)
        net_d = dev(net)
        r = decode.forwards_backwards_batch(net_d[:, :, :65], seqs, lengths=lens, full=full)
        assert r[1].shape == (net.shape[0], B, 65) and r[1].stride(1) == 65 + pad
        score, occ, row, prob = host(r)
        for b in range(B):
            assert same_results((score[b], occ[:lens[b], b], row[b], prob[b]), batch[b]), (pad, b)
            assert not occ[lens[b]:, b].any()                                              # rows the pair does not own
    # three launches: the limit that cuts the batch into three runs, by the rule of the *_many forms
    L = _lib.lib()
    alone = []
    for p, s in pairs:
        nrow, pos = np.array([p.shape[0]], np.int32), np.array([0, len(s)], np.int64)
        alone.append(int(L.slk_forward_backward_workspace_bytes(1, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p))))
    assert alone[1] == 256 + 8 * 40 * 256 and alone[6] == 256 + 8 * 8 * 1024               # 256 * ppt doubles per row
    limit = max(alone) + 120000
    assert len(transducer.workspace_runs([n - 248 for n in alone], limit - 512)) == 3
    split = run_packed(pairs, full=full, workspace_limit=limit)
    assert all(same_results(x, y) for x, y in zip(split, batch))
    with pytest.raises(ValueError, match=str(max(alone))):
        run_packed(pairs, full=full, workspace_limit=max(alone) - 1)


def test_same_bits_when_terms_collide():
    """Every position on one symbol, and positions on the blank's column: alone, in a batch, in the reverse order."""
    need_gpu()
    for full in (False, True):
        pairs = [build(n) for n in ("repeat", "blank_symbol", "small")]
        batch = run_packed(pairs, full=full)
        rev = run_packed(pairs[::-1], full=full)[::-1]
        assert all(same_results(x, y) for x, y in zip(batch, rev))
        for b in range(3):
            (alone,) = run_packed([pairs[b]], full=full)
            assert same_results(alone, batch[b])
        occ = batch[0][1]
        assert not occ[:, [0, 1, 2]].any() and (occ[:, 3] > 0).any()                       # `repeat` is all symbol 3


# ---- 5: structure -----------------------------------------------------------------------------------------------------------------

def test_structure():
    need_gpu()
    from sloika_amd import decode
    post = fc.make_post(8001, 5, 9, "float64")
    seq = fc.make_seq(8001, 9, 6, "random")
    for p in (post, post.astype(np.float32)):
        score, occ, row, prob = decode.forwards_backwards(p, [], full=True)                # no positions: every row stays
        assert np.array_equal(occ[:, -1], np.ones(5, p.dtype)) and not occ[:, :-1].any() and row.size == 0 and prob.size == 0
        assert score == decode.forwards(p, [], full=True)
        score, occ, row, prob = decode.forwards_backwards(p, seq, full=True)               # L = T + 1: no alignment
        assert score == -np.inf and not occ.any() and (row == -1).all() and not prob.any() and len(row) == 6
        score, occ, row, prob = decode.forwards_backwards(p, seq[:5], full=True)           # L = T: one alignment, every row moves
        assert np.isfinite(score) and row.tolist() == [0, 1, 2, 3, 4] and np.abs(prob - 1.0).max() < 1e-15
        assert np.abs(occ[np.arange(5), seq[:5]] - 1.0).max() < 1e-6 and abs(occ.sum() - 5.0) < 1e-5
        score, occ, row, prob = decode.forwards_backwards(p[:1], seq[:2])                  # T = 1
        t = fbr.forwards_backwards(p[:1], seq[:2], dtype=LD)
        assert np.abs(occ - t[1]).max() < (1e-15 if p.dtype == np.float64 else 1e-7) and np.array_equal(row, t[2])
    # a pair of no rows between two ordinary ones
    pairs = [(post, seq[:3]), (post[:0], seq[:2]), (post, seq[:4])]
    for full in (False, True):
        got = run_packed(pairs, full=full)
        assert got[1][0] == (-np.inf if full else 0.0) and got[1][1].shape == (0, 9)
        assert got[1][2].tolist() == [-1, -1] and got[1][3].tolist() == [0.0, 0.0]
        for b in (0, 2):
            (alone,) = run_packed([pairs[b]], full=full)
            assert same_results(alone, got[b])


# ---- 6: the C entry: what is written, and what is refused -------------------------------------------------------------------------

class Raw:
    """One call of slk_forward_backward_batch_f32 on the network layout [T][B][ld] with every output pre-filled with SENTINEL."""

    def __init__(self, post, lens, seqs, occ_ld=None, max_npos=None, short=0, blank=None, full=0):
        import torch
        from sloika_amd import _lib
        L = _lib.lib()
        T, B, ld = post.shape
        self.S = S = ld - 2                                                                # two pad columns behind nstate
        occ_ld = occ_ld or ld
        npos = [len(s) for s in seqs]
        pos = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
        nrow = np.asarray(lens, np.int32)
        post_d = dev(post)
        offs = dev(np.concatenate([np.arange(B, dtype=np.int64), pos]))
        ints = dev(np.concatenate([np.concatenate(seqs).astype(np.int32), nrow]))
        self.score = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
        self.occ = torch.full((T, B, occ_ld), SENTINEL, dtype=torch.float32, device="cuda")
        self.row = torch.full((int(pos[-1]),), -9, dtype=torch.int32, device="cuda")
        self.prob = torch.full((int(pos[-1]),), SENTINEL, dtype=torch.float64, device="cuda")
        self.need = int(L.slk_forward_backward_workspace_bytes(B, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p)))
        ws = torch.full((self.need,), 0x5A, dtype=torch.uint8, device="cuda")
        self.rc = L.slk_forward_backward_batch_f32(post_d.data_ptr(), ld, offs.data_ptr(), B, ints.data_ptr() + 4 * int(pos[-1]), S,
                                                   ints.data_ptr(), offs.data_ptr() + 8 * B, B, max(npos) if max_npos is None else max_npos,
                                                   S - 1 if blank is None else blank, full, 0.0, self.score.data_ptr(), self.occ.data_ptr(),
                                                   occ_ld, self.row.data_ptr(), self.prob.data_ptr(), ws.data_ptr(), self.need - short, stream())
        torch.cuda.synchronize()
        self.ws = ws.cpu().numpy()
        self.pos = pos
        self.score, self.occ, self.row, self.prob = (v.cpu().numpy() for v in (self.score, self.occ, self.row, self.prob))

    def pair(self, b, nr):
        return self.score[b], self.occ[:nr, b, :self.S], self.row[self.pos[b]:self.pos[b + 1]], self.prob[self.pos[b]:self.pos[b + 1]]


def raw_inputs():
    pairs = [(fc.make_post(8100 + i, T, 9, "float32"), fc.make_seq(8100 + i, 9, L, "random")) for i, (T, L) in enumerate([(12, 4), (7, 3), (12, 5)])]
    net, lens = network_layout(pairs, pad=2)
    return pairs, net, lens


def test_only_the_pairs_own_rows_and_columns_are_written():
    need_gpu()
    pairs, net, lens = raw_inputs()
    for occ_ld in (11, 16):
        r = Raw(net, lens, [s for _, s in pairs], occ_ld=occ_ld)
        assert r.rc == 0
        assert (r.occ[:, :, 9:] == SENTINEL).all()                                        # columns behind nstate
        for b in range(3):
            assert (r.occ[lens[b]:, b] == SENTINEL).all()                                  # rows behind lengths[b]
            (want,) = run_packed([pairs[b]])
            assert same_results(r.pair(b, lens[b]), want)


def test_refusals():
    need_gpu()
    from sloika_amd import decode, _lib
    pairs, net, lens = raw_inputs()
    seqs = [s for _, s in pairs]
    clean = Raw(net, lens, seqs)
    # a symbol that is no column: NaN for that pair only, nothing of it is written
    bad = [seqs[0], np.array([1, 9, 2]), seqs[2]]
    r = Raw(net, lens, bad)
    assert r.rc == 0 and np.isnan(r.score[1]) and (r.occ[:, 1] == SENTINEL).all()
    assert (r.row[r.pos[1]:r.pos[2]] == -9).all() and (r.prob[r.pos[1]:r.pos[2]] == SENTINEL).all()
    for b in (0, 2):
        assert same_results(r.pair(b, lens[b]), clean.pair(b, lens[b]))
    # a pair longer than max_npos said (5 positions against 4 under a budget of 2 states per thread is fine; 600 is not)
    long_seqs = [seqs[0], fc.make_seq(8200, 9, 600, "random"), seqs[2]]
    r = Raw(net, lens, long_seqs, max_npos=5)
    assert r.rc == 0 and np.isnan(r.score[1]) and (r.occ[:, 1] == SENTINEL).all() and (r.row[r.pos[1]:r.pos[2]] == -9).all()
    for b in (0, 2):
        assert same_results(r.pair(b, lens[b]), clean.pair(b, lens[b]))
    # a short workspace: the library's error code, and nothing is written, the workspace included
    r = Raw(net, lens, seqs, short=1)
    assert r.rc == _lib.SLK_ERR_WORKSPACE
    assert (r.score == SENTINEL).all() and (r.occ == SENTINEL).all() and (r.row == -9).all() and (r.prob == SENTINEL).all()
    assert (r.ws == 0x5A).all()
    # the limits of the host entry
    limit = decode.forward_max_positions()
    post = fc.make_post(8300, 3, 5, "float32")
    with pytest.raises(ValueError, match=str(limit)):
        decode.forwards_backwards(post, fc.make_seq(8300, 5, limit + 1, "random"))
    with pytest.raises(ValueError, match="8192"):
        decode.forwards_backwards_batch(np.zeros((1, 1, 8193), np.float32), [[1]])
    p = ctypes.c_void_p(256)                                                               # (never dereferenced: refused on the host)
    L = _lib.lib()
    assert L.slk_forward_backward_batch_f32(p, 8193, p, 1, p, 8193, p, p, 1, 3, 4, 0, 0.0, p, p, 8193, p, p, p, 1 << 20, None) == _lib.SLK_ERR_UNSUPPORTED
    assert L.slk_forward_backward_batch_f64(p, 5, p, 1, p, 5, p, p, 1, limit + 1, 4, 0, p, p, 5, p, p, p, 1 << 20, None) == _lib.SLK_ERR_UNSUPPORTED
    assert L.slk_forward_backward_batch_f32(p, 5, p, 1, p, 5, p, p, 1, 3, 4, 0, 0.0, p, p, 4, p, p, p, 1 << 20, None) == _lib.SLK_ERR_INVALID_ARG


def test_the_widest_table():
    """8192 columns: two tables of 64 KB in LDS."""
    need_gpu()
    post = fc.make_post(8400, 6, 8192, "float32")
    seq = fc.make_seq(8400, 8192, 4, "random")
    (score, occ, row, prob), = run_packed([(post, seq)])
    t = fbr.forwards_backwards(post, seq, dtype=LD)
    assert float(np.abs(occ - t[1]).max()) <= 2.0 ** -23 and np.array_equal(row, t[2])


# ---- 7: the pipeline --------------------------------------------------------------------------------------------------------------

def test_occupancy_chunks_end_to_end():
    """Convolution + Gru + Softmax(65), k = 3 (the model of the forward score's end-to-end test), three chunks of 200 samples."""
    torch = need_gpu()
    from sloika_amd import activation, bio, decode, layers, pipeline
    rs = np.random.RandomState(12)
    init = lambda shape: (rs.normal(size=shape) * 0.3).astype(np.float32)            # noqa: E731
    net = layers.Serial([layers.Convolution(1, 48, 11, 5, init=init, has_bias=True, fun=activation.tanh),
                         layers.Gru(48, 64, init=init, has_bias=True, fun=activation.tanh),
                         layers.Softmax(64, 65, init=init, has_bias=True)])
    bc = pipeline.Basecaller(net, kmer_len=3)
    chunks = dev(pipeline.synthetic_chunks(3, chunk_len=200, seed=12))
    letters = ["".join("ACGT"[v] for v in rs.randint(0, 4, size=n)) for n in (3, 9, 14)]
    states = [np.array([bio.kmer_mapping(3)[k] for k in bio.seq_to_kmers(s, 3)]) for s in letters]
    post = bc.posteriors(chunks).clone()
    for full in (True, False):
        by_states = host(bc.occupancy_chunks(chunks, states, full=full))
        by_letters = host(bc.occupancy_chunks(chunks, letters, full=full))
        direct = host(decode.forwards_backwards_batch(post, [s + 1 for s in states], full=full, blank=0, min_prob=bc.min_prob))
        ll = bc.score_chunks(chunks, states, full=full).cpu().numpy()
        assert by_states[1].shape == tuple(post.shape) and by_states[1].dtype == np.float32
        for other in (by_letters, direct):
            assert same(by_states[0], other[0]) and same(by_states[1], other[1])
            assert all(same(x, y) for x, y in zip(by_states[2], other[2])) and all(same(x, y) for x, y in zip(by_states[3], other[3]))
        assert same(by_states[0], ll) and np.isfinite(ll).all()
        assert np.abs(by_states[1].sum(axis=2) - 1.0).max() < 1e-5
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller(net, kmer_len=3, transducer=False, fused_decode=False).occupancy_chunks(chunks, letters)
