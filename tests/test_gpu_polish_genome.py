"""Polishing on genome coordinates on the device (csrc/polish_genome.hip through polish.letter_edits / read_windows / sum_gains /
rescore_genome / polish_genome, genome.Consensus.polish_variants; design/polish_genome.md).

The three kernels are compared integer for integer (the sum: bit for bit) with the plain loops of tests/polish_genome_ref.py.  The
scores of rescore_genome are pinned bit for bit to polish.rescore_drafts(band=) on the same rows, windows and centre lines, which is
itself pinned to extended precision (tests/test_gpu_rescore_band.py): no new tolerance.  The end-to-end case compares polish_genome with
the CPU model of tests/rescore_band_ref.py on the same posteriors, |device - model| <= 4 E_ref max(1, |model|) x support."""
import ctypes
import types

import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev, stream
from tests import polish_genome_ref as pg
from tests import rescore_ref as rr
from tests.rescore_gpu import E_REF

pytestmark = pytest.mark.gpu

ARRAYS = ("cand_pair", "cand_start", "cand_ndel", "cand_new_off", "cand_edit")


def random_letters(seed, n):
    rng = np.random.RandomState(seed)
    return ''.join('ACGT'[v] for v in rng.randint(0, 4, n))


def device_edits(genome, windows, klen, blank, mask, margin):
    import torch
    from sloika_amd import polish
    g = dev(np.frombuffer(genome.encode('ascii'), dtype=np.uint8).copy())
    w = np.array([(o, a, b, int(m)) for o, a, b, m in windows], dtype=np.int64).reshape(-1, 4)
    kinds = tuple(k for k in pg.KIND_NAMES if mask & pg.KIND_BITS[k])
    c = polish.letter_edits(g, dev(w[:, 0].copy()), dev(w[:, 1].copy()), dev(w[:, 2].copy()), dev(w[:, 3].astype(np.int32)), klen, blank,
                            kinds, margin)
    torch.cuda.synchronize()
    return c


def assert_edits_equal(c, want):
    assert np.array_equal(c.cand_off.cpu().numpy(), want["cand_off"]) and np.array_equal(c.pos_off.cpu().numpy(), want["pos_off"])
    n = int(want["cand_off"][-1])
    assert c.ncand == n
    for name in ARRAYS:
        assert np.array_equal(getattr(c, name).cpu().numpy()[:len(want[name])], want[name]), name
    nnew = int(want["cand_new_off"][-1])
    assert np.array_equal(c.cand_new.cpu().numpy()[:nnew], want["cand_new"])
    assert np.array_equal(c.seq.cpu().numpy()[:len(want["seq"])], want["seq"])


# ---- 1: candidates from letters ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("klen", [3, 5])
@pytest.mark.parametrize("n", [9, 40, 300])
def test_edits_equal_the_model(n, klen):
    """Windows of 9, 40 and 300 letters on both strands in one batch, blank 0; a second contig keeps the offsets honest."""
    need_gpu()
    genome = random_letters(3, 17) + random_letters(4, n + 11)
    windows = [(17, 5, 5 + n, False), (17, 5, 5 + n, True), (0, 2, 2 + min(n, 15), True)]
    for margin in (0, 2 * klen):
        assert_edits_equal(device_edits(genome, windows, klen, 0, 7, margin), pg.letter_edits(genome, windows, klen, 0, 7, margin))


def test_margin_leaves_nothing():
    need_gpu()
    genome = random_letters(5, 60)
    windows = [(0, 3, 12, False), (0, 20, 24, True)]                 # 9 letters under margin 5; 4 letters, no 5-mer
    c = device_edits(genome, windows, 5, 0, 7, 5)
    assert c.ncand == 0 and np.array_equal(c.cand_off.cpu().numpy(), [0, 0, 0])
    assert_edits_equal(c, pg.letter_edits(genome, windows, 5, 0, 7, 5))
    assert device_edits(genome, [(0, 3, 13, False)], 5, 0, 4, 5).ncand == 4      # ten letters: the insertions in front of letter 5 alone


@pytest.mark.parametrize("klen", [3, 5])
def test_runs_and_repeats(klen):
    """A homopolymer of 12, a dinucleotide repeat, runs touching either end of the window, a window of one letter: the prefix is
    followed along the run, and equal strings get equal triples."""
    need_gpu()
    a, b = random_letters(1, 20), random_letters(2, 17)
    for genome, w0, w1 in ((a + 'G' * 12 + b, 3, 46), (a + 'CA' * 9 + b, 2, 50), (a + 'T' * 7 + b, 4, 27), (a + 'T' * 7 + b, 20, 40),
                           ('A' * 30, 3, 25)):
        windows = [(0, w0, w1, False), (0, w0, w1, True)]
        c = device_edits(genome, windows, klen, 0, 7, 0)
        want = pg.letter_edits(genome, windows, klen, 0, 7, 0)
        assert_edits_equal(c, want)
        s = genome[w0:w1]
        seen = {}
        off = want["cand_new_off"]
        start, ndel, new = c.cand_start.cpu().numpy(), c.cand_ndel.cpu().numpy(), c.cand_new.cpu().numpy()
        for i, (kind, u, ch) in enumerate(pg.window_edits(s, klen, 7, 0)):
            trip = (int(start[i]), int(ndel[i]), tuple(new[off[i]:off[i + 1]]))
            assert seen.setdefault(pg.edited(s, kind, u, ch), trip) == trip


@pytest.mark.parametrize("mask", range(8))
def test_every_kinds_subset(mask):
    need_gpu()
    genome = random_letters(6, 20) + 'C' * 6 + random_letters(7, 20)
    windows = [(0, 4, 40, False), (0, 9, 44, True)]
    assert_edits_equal(device_edits(genome, windows, 3, 0, mask, 2), pg.letter_edits(genome, windows, 3, 0, mask, 2))


def test_overlapping_windows_feed_the_scoring_entry():
    """Seven windows of one contig that overlap, next to a second contig; blank 0.  The arrays go straight into
    slk_rescore_edits_banded_batch_f32: its grouping requirement is met (no SLK_ERR_INVALID_ARG) and every candidate is scored."""
    import torch
    from sloika_amd import _lib
    need_gpu()
    klen, S = 3, 65
    genome = random_letters(8, 23) + random_letters(9, 120)
    windows = [(23, 5 + 9 * i, 50 + 9 * i + (i % 3), i % 2 == 1) for i in range(7)] + [(0, 1, 22, False)]
    c = device_edits(genome, windows, klen, 0, 7, 2 * klen)
    want = pg.letter_edits(genome, windows, klen, 0, 7, 2 * klen)
    assert_edits_equal(c, want)
    pair = c.cand_pair.cpu().numpy()
    assert (np.diff(pair) >= 0).all() and set(pair) == set(range(8))
    nwin, T = len(windows), 70
    rng = np.random.default_rng(1)
    post = rng.uniform(0.05, 1.0, size=(T * nwin, S)).astype(np.float32)
    post /= post.sum(axis=1, keepdims=True)
    nrow = np.full(nwin, T, dtype=np.int32)
    L = _lib.lib()
    need = L.slk_rescore_edits_banded_workspace_bytes(nwin, nrow.ctypes.data_as(ctypes.c_void_p), 256)
    d = dict(post=dev(post), off=dev(np.arange(nwin, dtype=np.int64) * T), nrow=dev(nrow), lo=dev(np.zeros(nwin * (T + 1), np.int32)),
             boff=dev(np.arange(nwin + 1, dtype=np.int64) * (T + 1)))
    score = torch.full((nwin,), 7.0, dtype=torch.float64, device="cuda")
    ll = torch.full((c.ncand,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc = L.slk_rescore_edits_banded_batch_f32(d["post"].data_ptr(), S, d["off"].data_ptr(), 1, d["nrow"].data_ptr(), S, c.seq.data_ptr(),
                                              c.pos_off.data_ptr(), nwin, 0, 0.0, d["lo"].data_ptr(), d["boff"].data_ptr(), 256,
                                              c.cand_pair.data_ptr(), c.cand_start.data_ptr(), c.cand_ndel.data_ptr(),
                                              c.cand_new_off.data_ptr(), c.cand_new.data_ptr(), c.ncand, score.data_ptr(), ll.data_ptr(),
                                              ws.data_ptr(), need, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.isfinite(score.cpu().numpy()).all() and np.isfinite(ll.cpu().numpy()).all()


def test_a_letter_that_is_none_of_acgt_is_column_minus_one():
    need_gpu()
    genome = random_letters(10, 20) + 'N' + random_letters(11, 20)
    windows = [(0, 5, 35, False), (0, 5, 35, True)]
    c = device_edits(genome, windows, 3, 0, 6, 3)
    assert_edits_equal(c, pg.letter_edits(genome, windows, 3, 0, 6, 3))
    assert (c.seq.cpu().numpy() == -1).sum() == 6


# ---- 2: windows and centre lines -------------------------------------------------------------------------------------------------------

def window_batch(cases, klen, spoil=None):
    """polish.read_windows on hand-made alignments (align.Ops built by hand) -> (namespace, model results).  spoil: {read: what}."""
    import torch
    from sloika_amd import align, polish
    B = len(cases)
    spoil = spoil or {}
    ldq = max(c["ldq"] for c in cases)
    T = max(len(c["path"]) for c in cases) + 2
    paths, mrow = np.zeros((B, T), dtype=np.int32), np.full((B, T), -1, dtype=np.int32)
    lens, steps = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    codes, off, roff, rows, qlen = [], [0], [0], np.zeros((B, 9), dtype=np.int32), np.zeros(B, dtype=np.int32)
    want = []
    for b, c in enumerate(cases):
        c = dict(c)
        cd = c["codes"].copy()
        what = spoil.get(b)
        extra = 0
        if what == "code":
            cd[len(cd) // 2] = 7
        elif what == "move_row":
            c["move_row"] = c["move_row"].copy()
            c["move_row"][len(c["path"]) // 2] = c["move_row"][len(c["path"]) // 2 - 1] - 1
        elif what == "columns":
            extra = 2                                             # the slice of the column buffer disagrees with the row
        elif what == "letters":
            c["path"] = c["path"][:-1]
        paths[b, :len(c["path"])], mrow[b, :len(c["path"])] = c["path"], c["move_row"][:len(c["path"])]
        lens[b], steps[b], rows[b], qlen[b] = len(c["path"]), c["nrow"], c["row"], c["qlen"]
        codes.append(np.concatenate([cd, np.zeros(extra, np.uint8)]))
        off.append(off[-1] + len(cd) + extra)
        roff.append(roff[-1] + c["rlen"])
        want.append(pg.read_window(c["path"], c["move_row"], c["nrow"], c["qlen"], ldq, c["row"], cd, len(cd) + extra, c["minus"],
                                   c["wstart"], c["coff"], c["rlen"], 400, klen, c["nrow"] + 1))
    off = np.array(off, dtype=np.int64)
    q = torch.zeros((B, ldq), dtype=torch.uint8, device="cuda")
    part = (torch.zeros(int(roff[-1]), dtype=torch.uint8, device="cuda"), dev(np.array(roff, dtype=np.int64)), dev(rows),
            torch.zeros(B, dtype=torch.int32, device="cuda"))
    ops = align.Ops(q, ldq, dev(qlen), [part], rows, dev(np.concatenate(codes)), off, dev(off), np.zeros(B, dtype=np.int32))
    index = types.SimpleNamespace(offsets=np.array([0, cases[0]["coff"], 400], dtype=np.int64), G=400)
    info = {'contig': np.ones(B, dtype=np.int64), 'window_start': np.array([c["wstart"] for c in cases], dtype=np.int64)}
    strand = np.array(['-' if c["minus"] else '+' for c in cases])
    got = polish.read_windows(dev(paths), dev(lens), dev(mrow), dev(steps), ops, strand, info, index, klen)
    torch.cuda.synchronize()
    return got, want


def assert_windows_equal(got, want):
    center, coff = got.center.cpu().numpy(), got.center_off_host
    for b, (st, span, win, cen) in enumerate(want):
        assert got.status[b] == st, (b, got.status[b], st)
        mine = center[coff[b]:coff[b + 1]]
        if st != pg.DONE:                                            # its status and nothing else
            assert not got.span[b].any() and not got.window[b].any() and not mine.any(), b
            continue
        assert tuple(got.span[b]) == span and tuple(got.window[b]) == win, b
        assert np.array_equal(mine[:len(cen)], cen) and not mine[len(cen):].any(), b


@pytest.mark.parametrize("klen", [3, 5])
def test_windows_equal_the_model(klen):
    """Hand-made alignments on both strands with an insertion, a deletion, a mismatch and clipped ends; a read whose aligned part is
    the whole read; a window of 150 letters (more than two ballots of columns, more than two of rows)."""
    need_gpu()
    cases = [pg.planted_read(7, nwin=60, klen=klen), pg.planted_read(8, nwin=60, klen=klen, minus=True),
             pg.planted_read(9, nwin=40, klen=klen, whole=True), pg.planted_read(10, nwin=150, klen=klen, minus=True, clip=(70, 66)),
             pg.planted_read(11, nwin=64 + klen - 1, klen=klen, clip=(1, 1))]
    got, want = window_batch(cases, klen)
    assert [w[0] for w in want] == [pg.DONE] * len(cases)
    assert_windows_equal(got, want)
    # every centre line gives decode.band_lo a valid band
    from sloika_amd import decode
    center, coff = got.center, got.center_off_host
    for b, c in enumerate(cases):
        n = got.span[b, 1] - got.span[b, 0] + 1
        L = c["row"][4] - c["row"][3] - klen + 1
        lo = decode.band_lo(center[int(coff[b]):int(coff[b]) + int(n)], L, 256).cpu().numpy()
        assert np.array_equal(lo, pg.band_lo(want[b][3], L, 256))


def test_windows_refuse_bad_input():
    """One bad input of each kind between good reads: its status, nothing written for it, the neighbours as without it."""
    need_gpu()
    cases = [pg.planted_read(20 + i, nwin=50, klen=3, minus=i % 2 == 1) for i in range(6)]
    spoil = {1: "columns", 2: "code", 3: "move_row", 4: "letters"}
    got, want = window_batch(cases, 3, spoil)
    assert [w[0] for w in want] == [pg.DONE, pg.OPS, pg.BAD_CODE, pg.MOVE_ROW, pg.PATH, pg.DONE]
    assert_windows_equal(got, want)
    few = dict(cases[0])
    few["move_row"] = cases[0]["move_row"] // 8
    few["nrow"] = int(few["move_row"][-1]) + 1
    got, want = window_batch([few, cases[5]], 3)
    assert [w[0] for w in want] == [pg.FEW_ROWS, pg.DONE]
    assert_windows_equal(got, want)


# ---- 3: the sum ------------------------------------------------------------------------------------------------------------------------

def sum_case():
    """5 reads with staggered coverage of positions 10 .. 21: cells covered by one read, by none, a -inf and a NaN."""
    rng = np.random.default_rng(5)
    score = -rng.uniform(50.0, 60.0, size=5)
    pair, edit = [], []
    for r in range(5):
        for p in range(10 + 2 * r, 16 + 2 * r):
            for slot in range(8):
                if (p, slot) != (13, 6):                              # a cell nobody scores
                    pair.append(r)
                    edit.append(8 * p + slot)
    pair, edit = np.array(pair, dtype=np.int32), np.array(edit, dtype=np.int64)
    ll = score[pair] + rng.normal(0.0, 3.0, size=len(pair))
    ll[np.flatnonzero((edit == 8 * 14 + 2) & (pair == 1))] = -np.inf
    ll[np.flatnonzero((edit == 8 * 15 + 5) & (pair == 2))] = np.nan
    return score, ll, pair, edit


def python_sum(score, ll, pair, edit, lo, P):
    gain, support = np.zeros((P, 8)), np.zeros((P, 8), dtype=np.int32)
    for r in range(len(score)):                                      # read order, one float64 addition after the other
        for i in np.flatnonzero(pair == r):
            p, slot = divmod(int(edit[i]) - 8 * lo, 8)
            if not 0 <= p < P:
                continue
            if ll[i] != ll[i]:
                gain[p, slot] = np.nan
            elif np.isfinite(ll[i]):
                gain[p, slot] = gain[p, slot] + (ll[i] - score[r])
                support[p, slot] += 1
    return gain, support


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_sum_in_read_order():
    from sloika_amd import polish
    need_gpu()
    score, ll, pair, edit = sum_case()
    lo, P = 9, 14
    want_g, want_s = python_sum(score, ll, pair, edit, lo, P)
    model_g, model_s = pg.sum_gains(score, ll, pair, edit, lo, P)
    assert np.array_equal(model_s, want_s) and same_bits(np.nan_to_num(model_g, nan=-1.0), np.nan_to_num(want_g, nan=-1.0))
    gain, support = polish.sum_gains(dev(score), dev(ll), dev(pair), dev(edit), lo, P)
    gain, support = gain.cpu().numpy(), support.cpu().numpy()
    assert np.array_equal(support, want_s)
    assert np.isnan(gain[15 - lo, 5]) and np.isnan(want_g[15 - lo, 5]) and np.isnan(gain).sum() == 1
    assert same_bits(np.nan_to_num(gain, nan=-1.0), np.nan_to_num(want_g, nan=-1.0))
    assert gain[13 - lo, 6] == 0.0 and support[13 - lo, 6] == 0                     # covered by none
    assert support[10 - lo, 0] == 1 and support[14 - lo, 2] == 2                    # by one read; the -inf of read 1 is not counted
    assert support.max() == 3
    # the candidates handed over in reversed pair-block order
    rev = np.concatenate([np.flatnonzero(pair == r) for r in range(4, -1, -1)])
    g2, s2 = polish.sum_gains(dev(score), dev(ll[rev]), dev(pair[rev]), dev(edit[rev]), lo, P)
    assert np.array_equal(s2.cpu().numpy(), support) and same_bits(np.nan_to_num(g2.cpu().numpy(), nan=-1.0), np.nan_to_num(gain, nan=-1.0))
    # a batch split into two launches that come in read order
    first = pair < 2
    g3, s3 = polish.sum_gains(dev(score), dev(ll[first]), dev(pair[first]), dev(edit[first]), lo, P)
    g3, s3 = polish.sum_gains(dev(score), dev(ll[~first]), dev(pair[~first]), dev(edit[~first]), lo, P, g3, s3)
    assert np.array_equal(s3.cpu().numpy(), support) and same_bits(np.nan_to_num(g3.cpu().numpy(), nan=-1.0), np.nan_to_num(gain, nan=-1.0))
    # a slice of the region is the slice of the whole
    g4, s4 = polish.sum_gains(dev(score), dev(ll), dev(pair), dev(edit), 12, 5)
    assert np.array_equal(s4.cpu().numpy(), support[3:8]) and same_bits(np.nan_to_num(g4.cpu().numpy(), nan=-1.0),
                                                                        np.nan_to_num(gain[3:8], nan=-1.0))


# ---- 4: the planted genome -------------------------------------------------------------------------------------------------------------

MIN_PROB = 1e-5


def called(sample):
    """The planted posteriors on the device, decoded by the real decoder."""
    from sloika_amd import decode
    post, steps = dev(sample["post"]), dev(sample["steps"])
    _, paths, lens, move_row, _, _ = decode.viterbi_marginals_batch(post, sample["k"], min_prob=MIN_PROB, lengths=steps)
    return post, steps, paths, lens, move_row


@pytest.fixture(scope="module")
def planted():
    need_gpu()
    from sloika_amd import genome
    s = pg.planted_genome()
    post, steps, paths, lens, move_row = called(s)
    idx = genome.Index([("draft", s["draft"])], k=14)
    keep = np.arange(len(s["texts"])) != 13
    return dict(sample=s, call=(post, steps, paths, lens, move_row), idx=idx, keep=keep)


def test_scores_are_rescore_drafts_bit_for_bit():
    """Windows of fewer than 255 k-mers at W = 256 (lo all 0): every read's score and every ll_edit - score of rescore_genome are the
    bits polish.rescore_drafts(band=) returns for the read's rows, its window's string and the same centre line; edits are matched
    through cand_edit."""
    need_gpu()
    import torch
    from sloika_amd import bio, genome, polish
    s = pg.planted_genome(seed=4, windows=pg.SHORT_WINDOWS)
    k = s["k"]
    post, steps, paths, lens, move_row = called(s)
    idx = genome.Index([("draft", s["draft"])], k=14)
    res, strand, info, _, ops = idx.map_paths(paths, lens, k, ops=True)
    got = polish.rescore_genome(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256)
    nread = len(pg.SHORT_WINDOWS)
    assert got.status.tolist() == [polish.READ_DONE] * nread + [polish.READ_UNMAPPED, polish.READ_DONE]
    w = polish.read_windows(paths, lens, move_row, steps, ops, strand, info, idx, k)
    center = w.center.cpu().numpy()
    score = got.score.cpu().numpy()
    cand_read, cand_edit, ll = got.cand_read.cpu().numpy(), got.cand_edit.cpu().numpy(), got.ll_edit.cpu().numpy()
    host = s["post"]
    compared = 0
    for r in np.flatnonzero(got.status == polish.READ_DONE):
        r0, r1 = (int(v) for v in got.span[r])
        w0, w1 = (int(v) for v in got.window[r])
        minus = strand[r] == '-'
        text = pg.window_string(s["draft"], 0, w0, w1, minus)
        assert len(text) - k + 1 < 255
        cen = center[w.center_off_host[r]:w.center_off_host[r] + r1 - r0 + 1]
        rows = np.ascontiguousarray(host[r0:r1, r, :])
        ref = polish.rescore_drafts(dev(rows), [text], k, blank=0, row_off=np.array([0, r1 - r0]), band=([cen], 256))[0]
        assert same_bits(ref.score.item(), score[r]), r
        gain = ref.gain.cpu().numpy()
        mine = dict((int(e), float(v)) for e, v in zip(cand_edit[cand_read == r], ll[cand_read == r]))
        assert len(mine) == pg.count(len(text), k, 7, 2 * k)
        for (kind, u, c, _), g in zip(ref.edits, gain):
            fu, fc = pg.forward_edit(len(text), minus, kind, u, c)
            key = 8 * (w0 + fu) + pg.slot_of(kind, fc, s["draft"][w0 + fu] if kind == 'sub' else '')
            if key in mine and (2 * k <= u <= len(text) - 2 * k):
                assert same_bits(mine[key] - score[r], g), (r, kind, u, c)
                compared += 1
        assert compared
    assert compared == len(ll)


def model_round(text, k, call, host_post, mapping, keep, width=256):
    """One round of the CPU model on the device's mapping of the calls: tests/polish_genome_ref.py for windows, centre lines,
    candidates and the sum, tests/rescore_band_ref.evaluate (float64) for the scores.
    -> (gain [P][8], support, reads used, per cell the sum of max(1, |score|) over the reads counted)"""
    from tests import rescore_band_ref as rb
    res, strand, info, ops = mapping
    paths, lens, move_row, steps = (v.cpu().numpy() for v in call)
    qlen = ops.query_lengths()
    score = np.full(len(steps), np.nan)
    pairs, edits, lls, used = [], [], [], []
    for r in range(len(steps)):
        if info['contig'][r] < 0 or not keep[r]:
            continue
        rlen = int(info['window_end'][r] - info['window_start'][r])
        codes = ops.codes(r)
        st, span, win, cen = pg.read_window(paths[r, :lens[r]].tolist(), move_row[r], int(steps[r]), int(qlen[r]), ops.ldq, ops.rows[r], codes,
                                            len(codes), strand[r] == '-', int(info['window_start'][r]), 0, rlen, len(text), k,
                                            int(steps[r]) + 1)
        if st != pg.DONE:
            continue
        used.append(r)
        c = pg.letter_edits(text, [(0, win[0], win[1], strand[r] == '-')], k, 0, 7, 2 * k)
        off = c["cand_new_off"]
        trip = [(int(a), int(d), c["cand_new"][off[i]:off[i + 1]]) for i, (a, d) in enumerate(zip(c["cand_start"], c["cand_ndel"]))]
        lo = rb.band_lo(cen, len(c["seq"]), width)
        rows = host_post[span[0]:span[1], r, :]
        sc, ll = rb.evaluate(rows, c["seq"], trip, lo, width, 0, np.float64)
        score[r] = float(sc)
        pairs += [r] * len(trip)
        edits += c["cand_edit"].tolist()
        lls += [float(v) for v in ll]
    lls, pairs, edits = np.array(lls), np.array(pairs, dtype=np.int32), np.array(edits, dtype=np.int64)
    gain, support = pg.sum_gains(score, lls, pairs, edits, 0, len(text))
    # per cell the sum over the reads counted of max(1, |score|): what a gain's bound is made of
    size = np.maximum(1.0, np.abs(score[pairs]))
    scale, _ = pg.sum_gains(score, np.where(np.isfinite(lls), score[pairs] + size, lls), pairs, edits, 0, len(text))
    return gain, support, used, scale


def test_polish_genome_returns_the_truth(planted):
    """12 planted reads on a draft with a substitution, a letter missing from a homopolymer and a letter too many: polish_genome returns
    the truth, every planted difference is applied with support >= 3 and nothing else is; the unmapped read and the one failing keep
    are in the status.  Round 0 against the CPU model fed the same posteriors and the device's mapping: the same cells chosen, gains
    within 4 E_ref max(1, |value|) x support.  A gain is a sum over `support` reads of ll_edit - score, and `value` is what each
    side of that difference is bounded by in tests/test_gpu_rescore_band.py: the read's score (an ll_edit is within a few units of
    it).  So the bound of a cell is 4 E_ref x the sum of max(1, |score|) over the reads counted; with every score equal that is the
    bound's wording.  It cannot be read with |value| = |gain|: a difference of two float64 numbers of size 1300 is no better than their
    rounding, 1.1e-13 each, whatever computes it.  Measured on an MI355X over the 4708 cells a read scored (scores about -1300): largest
    distance 4.55e-13; 0.046 of E_ref x the sum of max(1, |score|) (bound 4), and 10.9 of E_ref max(1, |gain|) x support, the reading
    that float64 cannot meet."""
    from sloika_amd import bio, genome, polish
    s, call, idx, keep = planted["sample"], planted["call"], planted["idx"], planted["keep"]
    post, steps, paths, lens, move_row = call
    k = s["k"]
    out, last = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, keep=keep)
    assert len(out) == 1 and out[0].name == "draft"
    assert out[0].sequence == s["truth"]
    assert last.status.tolist() == [polish.READ_DONE] * 12 + [polish.READ_UNMAPPED, polish.READ_NOT_KEPT]      # the reads used, all of them
    applied = out[0].applied
    assert len(applied) == 3 and out[0].rounds == 1 and all(a[0] == 0 for a in applied)
    by_kind = dict((a[2], a) for a in applied)
    assert by_kind['sub'][1:4] == (pg.SAMPLE_SUB, 'sub', s["truth"][pg.SAMPLE_SUB])
    assert by_kind['ins'][3] == 'A' and 300 <= by_kind['ins'][1] <= 304
    assert by_kind['del'][1] == 449
    assert all(a[4] > 0.0 and a[5] >= 3 for a in applied)
    # round 0 again, beside the model
    res, strand, info, _, ops = idx.map_paths(paths, lens, k, ops=True)
    first = polish.rescore_genome(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256, keep=keep)
    gain, support, used, scale = model_round(s["draft"], k, (paths, lens, move_row, steps), s["post"], (res, strand, info, ops), keep)
    assert used == list(range(12))
    dg, ds = first.gain.cpu().numpy(), first.support.cpu().numpy()
    assert np.array_equal(ds, support)
    assert np.array_equal(np.isnan(dg), np.isnan(gain)) and not np.isnan(dg).any()
    fin = np.isfinite(gain)
    assert np.array_equal(np.isfinite(dg), fin)
    assert not dg[support == 0].any() and not gain[support == 0].any()
    fin = fin & (support > 0)
    diff = np.abs(dg[fin] - gain[fin])
    worst = float((diff / (E_REF * scale[fin])).max())
    naive = float((diff / (E_REF * np.maximum(1.0, np.abs(gain[fin])) * np.maximum(support[fin], 1))).max())
    print("polish_genome: largest |device - model| of a gain %.3g over %d cells, scores about %.0f: %.3f of E_ref x (sum of max(1, |score|) "
          "over the reads counted); %.3f of E_ref max(1, |gain|) support" % (float(diff.max()), int(fin.sum()), float(scale.max() / 12), worst, naive))
    assert worst <= 4.0
    text = {"draft": s["draft"]}
    cells = [first.edit_of(p, q) + (float(gain[p, q]), int(support[p, q])) for p, q in zip(*np.nonzero((gain > 0.0) & (support >= 2)))]
    want = polish.accept_genome_edits(cells, text, k)
    assert sorted((t[1], t[2], t[3]) for t in want) == sorted((a[1], a[2], a[3]) for a in applied)
    # with min_support above the coverage nothing is applied
    none, _ = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, keep=keep, min_support=13,
                                   max_rounds=1)
    assert none[0].sequence == s["draft"] and none[0].applied == [] and none[0].rounds == 0


def test_batching_region_and_absent_reads_change_no_bit(planted):
    """gain and support do not depend on how the reads are cut into launches, on the region being the whole genome or a slice, or on
    the unmapped read and the read failing keep being there at all."""
    from sloika_amd import polish
    s, call, idx, keep = planted["sample"], planted["call"], planted["idx"], planted["keep"]
    post, steps, paths, lens, move_row = call
    k = s["k"]
    res, strand, info, _, ops = idx.map_paths(paths, lens, k, ops=True)
    run = lambda **kw: polish.rescore_genome(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256, **kw)     # noqa: E731
    whole = run(keep=keep)
    g, sp = whole.gain.cpu().numpy(), whole.support.cpu().numpy()
    assert sp.max() >= 6 and np.isfinite(g).all()
    nrow = (whole.span[:12, 1] - whole.span[:12, 0]).astype(np.int64)
    limit = int(16 * (nrow.max() + 1) * 257 * 5)                     # room for about five pairs: three launches or more
    split = run(keep=keep, workspace_limit=limit)
    assert same_bits(split.gain.cpu().numpy(), g) and np.array_equal(split.support.cpu().numpy(), sp)
    part = run(keep=keep, region=("draft", 140, 460))
    assert same_bits(part.gain.cpu().numpy(), g[140:460]) and np.array_equal(part.support.cpu().numpy(), sp[140:460])
    both = run()                                                     # read 13 spells read 0's window: it adds to read 0's cells only
    b = both.support.cpu().numpy()
    assert both.status[13] == polish.READ_DONE and (b - sp).max() == 1 and (b - sp).min() == 0
    w0, w1 = (int(v) for v in both.window[13])
    assert not (b - sp)[:w0].any() and not (b - sp)[w1 + 1:].any()


def test_variants_join():
    """The planted pileup of tests/pileup_cases.py, its reads as planted posteriors: polish_variants puts a positive gain beside each
    planted single-letter variant and names the two-letter insertion as not a single-letter edit."""
    need_gpu()
    from sloika_amd import decode, genome, polish
    from tests import pileup_cases
    case = pileup_cases.planted()
    k = 3
    rng = np.random.default_rng(2)
    reads = case['reads']
    steps = np.array([2 * (len(t) - k + 1) for t in reads], dtype=np.int32)
    host = rng.uniform(size=(int(steps.max()), len(reads), 65)).astype(np.float32) * np.float32(0.2)
    host[:, :, 0] += 1.0
    for r, t in enumerate(reads):
        states = np.array(rr.states_of(t, k))
        rows = np.sort(rng.choice(int(steps[r]), size=len(states), replace=False))
        host[rows, r, 0] -= 1.0
        host[rows, r, states + 1] += 1.0
    host /= host.sum(axis=2, keepdims=True)
    post, steps_d = dev(host), dev(steps)
    _, paths, lens, move_row, _, _ = decode.viterbi_marginals_batch(post, k, min_prob=MIN_PROB, lengths=steps_d)
    idx = genome.Index([(pileup_cases.CONTIG, case['genome'])], k=8, bin_width=512)
    res, strand, info, _, ops = idx.map_paths(paths, lens, k, ops=True)
    pile, cons = genome.pileup(idx, res, strand, info, ops)
    got = polish.rescore_genome(post, steps_d, paths, lens, move_row, idx, res, strand, info, ops, k, width=256)
    assert (got.status == polish.READ_DONE).sum() >= 60
    rows = cons.polish_variants(got)
    assert [v[:5] for v in rows] == case['variants']
    by = dict(((v[1], v[2]), v) for v in rows)
    single = [v for v in case['variants'] if v[2] == 'sub' or (v[2] == 'ins' and len(v[4]) == 1) or (v[2] == 'del' and v[3] == 'A' and
                                                                                                   case['genome'][v[1] + 1] == 'A')]
    assert len(single) == 3
    for v in single:
        gain, support, one = by[(v[1], v[2])][-3:]
        assert one and support >= 3 and gain > 0.0, v
    longer = [v for v in rows if v[2] == 'ins' and len(v[4]) == 2]
    assert len(longer) == 1 and longer[0][-3:] == (None, 0, False)
    assert all(v[-1] and v[-2] >= 3 and np.isfinite(v[-3]) for v in rows if v[2] == 'del')


def test_basecaller_rescore_and_polish_genome():
    """Two synthetic reads through a small built model, the genome a stretch of each read's own call: Basecaller.rescore_genome is
    polish.rescore_genome on the posterior, the calls and the mapping of the same reads, bit for bit; reads whose band cannot be laid are
    reported, not raised, and polish_genome then applies nothing."""
    need_gpu()
    import torch
    from sloika_amd import bio, genome, models, pipeline, polish
    net = models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=7))
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    base = pipeline.synthetic_chunks(2, chunk_len=3000, seed=21)
    reads = [base[0], base[1][:2200]]
    _, paths, lens, move_row, _, _, _ = bc.call_reads_qual(reads)
    calls = bio.paths_to_bases(paths, lens, 5)
    idx = genome.Index([("a", calls[0][20:144]), ("b", calls[1][10:94])], k=14)
    got = bc.rescore_genome(reads, idx, width=256)
    padded, ns = bc._padded_reads(reads, (0, 0), 0.0, None, "test")
    post, steps = bc._read_posteriors(padded, ns)
    res, strand, info, _, ops = idx.map_paths(paths, lens, 5, ops=True)
    want = polish.rescore_genome(post, steps, paths, lens, move_row, idx, res, strand, info, ops, 5, width=256, blank=0, min_prob=bc.min_prob)
    assert info['contig'].tolist() == [0, 1] and got.status.tolist() == want.status.tolist()
    assert got.window.tolist() == want.window.tolist() and got.span.tolist() == want.span.tolist()
    bits = lambda t: t.cpu().numpy().tobytes()                    # noqa: E731
    assert torch.equal(got.support, want.support) and bits(got.gain) == bits(want.gain) and bits(got.score) == bits(want.score)
    print("rescore_genome on a random network's own calls: status %s, windows %s, rows %s, cells scored %d"
          % (got.status.tolist(), got.window.tolist(), got.span.tolist(), int((got.support > 0).sum())))
    # a random network's own call has more k-mers than its read has rows (design/rescore_band.md 6): no band can be laid, which is
    # reported per read and never raised; nothing is scored and nothing applied
    assert got.status.tolist() == [pg.FEW_ROWS] * 2 and not bool(got.support.any()) and not bool(got.gain.any())
    assert bool(torch.isnan(got.score).all()) and got.edits() == [] and got.top(3) == []
    out, last = bc.polish_genome(reads, idx, width=256, min_support=1, max_rounds=2)
    assert [(o.name, o.sequence, o.applied, o.rounds) for o in out] == [("a", calls[0][20:144], [], 0), ("b", calls[1][10:94], [], 0)]
    assert last.status.tolist() == got.status.tolist()
    print("polish_genome on a random network's own calls: %s edits applied" % [len(o.applied) for o in out])
