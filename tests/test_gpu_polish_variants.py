"""Proposed variants of any length on genome coordinates, on the device (csrc/polish_variants.hip through polish.variant_edits /
sum_variant_gains / repeat_variants / rescore_variants / polish_genome(proposals=), genome.Consensus.polish_variants,
pipeline.Basecaller.rescore_variants; design/polish_variants.md).

The candidate and proposer kernels are compared integer for integer, the sum bit for bit, with the plain loops of
tests/polish_variants_ref.py.  The scores of rescore_variants are pinned bit for bit to decode.rescore_edits_banded_batch on the same
rows, window strings, centre lines and the model's triples, which is itself pinned to extended precision
(tests/test_gpu_rescore_band.py): no new tolerance.  The planted case compares the gains with the float64 CPU model of
tests/rescore_band_ref.py on the same posteriors, |device - model| <= 4 E_ref x the sum of max(1, |score|) over the reads counted: the
bound tests/test_gpu_polish_genome.py applies to its planted case."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev
from tests import polish_genome_ref as pg
from tests import polish_variants_ref as pv
from tests import rescore_ref as rr
from tests.rescore_gpu import E_REF

pytestmark = pytest.mark.gpu

ARRAYS = ("cand_pair", "cand_start", "cand_ndel", "cand_new_off")
MIN_PROB = 1e-5


def random_letters(seed, n, letters='ACGT'):
    rng = np.random.RandomState(seed)
    return ''.join(letters[v] for v in rng.randint(0, len(letters), n))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def make_set(variants, contig_off, index=None):
    """A polish.VariantSet of packed-offset rows (contig offset, pos, ndel, alt) in the caller's order, sorted as the host wrapper
    sorts.  -> (set, the sorted rows, order)"""
    from sloika_amd import polish
    rows, order = pv.sort_variants(variants)
    text = ''.join(v[3] for v in rows)
    vs = polish.VariantSet(index, dev(np.array([v[0] for v in rows], dtype=np.int64)), dev(np.array([v[1] for v in rows], dtype=np.int64)),
                           dev(np.array([v[2] for v in rows], dtype=np.int32)),
                           dev(np.concatenate([[0], np.cumsum([len(v[3]) for v in rows])]).astype(np.int64)),
                           dev(np.frombuffer(text.encode('ascii'), dtype=np.uint8).copy()), dev(np.array(contig_off, dtype=np.int64)),
                           np.array(order, dtype=np.int64))
    return vs, rows, order


def device_edits(genome, windows, vs, klen, margin, blank=0):
    import torch
    from sloika_amd import polish
    g = dev(np.frombuffer(genome.encode('ascii'), dtype=np.uint8).copy())
    w = np.array([(o, a, b, int(m)) for o, a, b, m in windows], dtype=np.int64).reshape(-1, 4)
    c = polish.variant_edits(g, vs.contig_off, dev(w[:, 0].copy()), dev(w[:, 1].copy()), dev(w[:, 2].copy()), dev(w[:, 3].astype(np.int32)),
                             vs, klen, blank, margin)
    torch.cuda.synchronize()
    return c


def assert_edits_equal(c, want, order):
    assert np.array_equal(c.cand_off.cpu().numpy(), want["cand_off"]) and np.array_equal(c.pos_off.cpu().numpy(), want["pos_off"])
    assert c.ncand == int(want["cand_off"][-1])
    for name in ARRAYS:
        assert np.array_equal(getattr(c, name).cpu().numpy()[:len(want[name])], want[name]), name
    assert np.array_equal(c.cand_var_sorted.cpu().numpy(), want["cand_var"])
    order = np.asarray(order, dtype=np.int64)
    assert np.array_equal(c.cand_var.cpu().numpy(), order[want["cand_var"]] if len(order) else want["cand_var"])
    nnew = int(want["cand_new_off"][-1])
    assert np.array_equal(c.cand_new.cpu().numpy()[:nnew], want["cand_new"])
    assert np.array_equal(c.seq.cpu().numpy()[:len(want["seq"])], want["seq"])
    status = np.zeros(len(order), dtype=np.int32)
    status[order] = want["var_status"]
    assert np.array_equal(c.var_status.cpu().numpy(), status)


def check(genome, contig_off, windows, variants, klen, margin):
    vs, rows, order = make_set(variants, contig_off)
    c = device_edits(genome, windows, vs, klen, margin)
    want = pv.variant_edits(genome, contig_off, windows, rows, klen, 0, margin)
    assert_edits_equal(c, want, order)
    return c, want, rows


def random_variants(seed, off, lo, hi, count, klen, letters='ACGT'):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        pos = int(rng.randint(lo, hi + 1))
        ndel = int(rng.randint(0, min(4, hi - pos) + 1))
        alt = ''.join(letters[v] for v in rng.randint(0, len(letters), int(rng.randint(0, pv.max_alt(klen) + 1))))
        out.append((off, pos, ndel, alt))
    return out


# ---- 1: candidates from variants -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("klen", [3, 5])
@pytest.mark.parametrize("n", [9, 40, 300])
def test_candidates_equal_the_model(n, klen):
    """Windows of 9, 40 and 300 letters on both strands in one batch, margins 0, 2 and 2 k; a second contig keeps the offsets honest.
    Random variants (several at one position; some empty or equal to the reference, which are refused), a variant whose far end is
    exactly at w1 - margin and one a letter beyond, insertions at w0 + margin and at w1 - margin."""
    need_gpu()
    genome = random_letters(3, 17) + random_letters(4, n + 11)
    contig_off = [0, 17, 17 + n + 11]
    windows = [(17, 5, 5 + n, False), (17, 5, 5 + n, True), (0, 2, 2 + min(n, 15), True)]
    scored = 0
    for margin in (0, 2, 2 * klen):
        w0, w1 = 5 + margin, 5 + n - margin
        variants = random_variants(n + klen, 17, 0, n + 11, 3 * n, klen) + random_variants(n, 0, 0, 17, 12, klen)
        if w1 - 3 >= w0:
            variants += [(17, w1 - 3, 3, 'G'), (17, w1 - 3, 4, 'G'), (17, w1 - 2, 2, ''), (17, w1 - 2, 3, '')]
        if w1 >= w0:
            variants += [(17, w0, 0, 'TG'), (17, w1, 0, 'CA'), (17, w1, 0, 'ACGTAC'[:pv.max_alt(klen)]), (17, w0, 0, 'G'), (17, w1 + 1, 0, 'G'),
                         (17, max(w0 - 1, 0), 0, 'G')]
        c, want, _ = check(genome, contig_off, windows, variants, klen, margin)
        scored += c.ncand
    assert scored > 0 or n < 2 * klen


def test_no_variant_and_more_than_two_waves():
    """A window with no variant in range beside windows with more than 130: the wave loop makes two full passes and a ragged one."""
    need_gpu()
    genome = random_letters(5, 400)
    variants = random_variants(7, 0, 100, 300, 150, 3)
    windows = [(0, 0, 60, False), (0, 100, 300, False), (0, 100, 300, True), (0, 310, 400, True), (0, 90, 310, False)]
    c, want, _ = check(genome, [0, 400], windows, variants, 3, 0)
    counts = np.diff(want["cand_off"])
    assert counts[0] == 0 and counts[3] == 0 and counts[1] > 130 and counts[1] % 64 and counts[4] >= counts[1]
    c, want, _ = check(genome, [0, 400], windows, [], 3, 0)          # no variant at all
    assert c.ncand == 0
    c, want, _ = check(genome, [0, 400], [], variants, 3, 0)         # no window at all
    assert c.ncand == 0


@pytest.mark.parametrize("klen", [3, 5])
def test_units_of_a_tract_at_the_window_ends(klen):
    """Deleting one unit of (AC)x9 at the window's front, middle and very end, the window the tract itself: dF / dB run to the
    window's ends and come back none.  Equal strings get equal triples."""
    need_gpu()
    a = random_letters(1, 20)
    genome = a + 'AC' * 9 + random_letters(2, 17)
    variants = [(0, 20, 2, ''), (0, 28, 2, ''), (0, 36, 2, ''), (0, 20, 0, 'AC'), (0, 38, 0, 'AC'), (0, 29, 0, 'CA'), (0, 20, 4, ''),
                (0, 21, 2, ''), (0, 35, 2, 'G')]
    for w0, w1 in ((20, 38), (19, 38), (20, 40), (3, 50)):
        windows = [(0, w0, w1, False), (0, w0, w1, True)]
        c, want, rows = check(genome, [0, len(genome)], windows, variants, klen, 0)
        off = want["cand_new_off"]
        for b in (0, 1):
            s, seen = pg.window_string(genome, *windows[b]), {}
            for i in np.flatnonzero(want["cand_pair"] == b):
                u, ndel, alt = pv.window_edit(windows[b], rows[want["cand_var"][i]])
                trip = (int(want["cand_start"][i]), int(want["cand_ndel"][i]), tuple(want["cand_new"][off[i]:off[i + 1]]))
                assert seen.setdefault(s[:u] + alt + s[u + ndel:], trip) == trip
            assert len(seen) < (want["cand_pair"] == b).sum()


def test_contigs_boundaries_and_overlaps():
    """Two contigs whose windows have the same local coordinates; an insertion at the contigs' boundary belonging to either side, at
    margin 0; seven overlapping windows of one contig; a letter that is none of ACGT beside a variant gives column -1."""
    need_gpu()
    genome = random_letters(8, 40) + random_letters(9, 120)
    contig_off = [0, 40, 160]
    variants = [(0, 40, 0, 'AC'), (40, 0, 0, 'GT'), (0, 12, 2, 'T'), (40, 12, 2, 'T'), (0, 12, 0, 'GG'), (40, 12, 3, '')]
    windows = [(0, 5, 30, False), (40, 5, 30, False), (0, 20, 40, False), (0, 20, 40, True), (40, 0, 10, False), (40, 0, 10, True)]
    c, want, rows = check(genome, contig_off, windows, variants, 3, 0)
    by_window = [sorted(rows[v][:2] for v in want["cand_var"][want["cand_pair"] == b]) for b in range(len(windows))]
    assert by_window[0] == [(0, 12), (0, 12)] and by_window[1] == [(40, 12), (40, 12)]
    assert by_window[2] == by_window[3] == [(0, 40)] and by_window[4] == by_window[5] == [(40, 0)]
    many = random_variants(11, 40, 0, 120, 90, 3)
    overlapping = [(40, 5 + 9 * i, 50 + 9 * i + (i % 3), i % 2 == 1) for i in range(7)] + [(0, 1, 22, False)]
    c, want, _ = check(genome, contig_off, overlapping, many + variants, 3, 2 * 3)
    pair = c.cand_pair.cpu().numpy()
    assert (np.diff(pair) >= 0).all() and len(set(pair)) >= 7
    other = genome[:70] + 'N' + genome[71:]
    c, want, _ = check(other, contig_off, [(40, 10, 60, False), (40, 10, 60, True)], [(40, 31, 0, 'AC'), (40, 27, 2, ''), (40, 50, 0, 'AC')],
                       3, 0)
    new = c.cand_new.cpu().numpy()[:int(want["cand_new_off"][-1])]
    assert (new == -1).any() and (new >= 0).any() and (c.seq.cpu().numpy() == -1).sum() == 6


def test_candidates_feed_the_scoring_entry():
    """The arrays go straight into decode.rescore_edits_banded_device: its grouping requirement is met and every candidate is scored."""
    import torch
    from sloika_amd import decode
    need_gpu()
    klen, S, T = 3, 65, 90
    genome = random_letters(8, 23) + random_letters(9, 120)
    windows = [(23, 5 + 9 * i, 50 + 9 * i + (i % 3), i % 2 == 1) for i in range(7)] + [(0, 1, 22, False)]
    variants = random_variants(13, 23, 0, 120, 80, klen) + random_variants(14, 0, 0, 23, 10, klen)
    c, want, _ = check(genome, [0, 23, 143], windows, variants, klen, klen)
    nwin = len(windows)
    rng = np.random.default_rng(1)
    post = dev(rng.uniform(0.05, 1.0, size=(T, nwin, S)).astype(np.float32))
    band = torch.zeros(nwin * (T + 1), dtype=torch.int32, device=post.device)
    score, ll = decode.rescore_edits_banded_device(post, np.arange(nwin, dtype=np.int64), nwin, np.full(nwin, T, dtype=np.int32), c.seq,
                                                   c.pos_off, band, 256, c.cand_off_host, c.cand_pair, c.cand_start, c.cand_ndel,
                                                   c.cand_new_off, c.cand_new, blank=0)
    assert c.ncand > 40 and bool(torch.isfinite(score).all()) and bool(torch.isfinite(ll).all())


# ---- 2: refusals ---------------------------------------------------------------------------------------------------------------------

GOOD = [(0, 3, 2, ''), (0, 9, 0, 'AC'), (0, 20, 1, 'G'), (30, 2, 0, 'TT'), (30, 11, 3, 'A'), (30, 15, 1, '')]


def spoiled(what):
    """GOOD on the device with one entry spoiled -> (set, the entry, its status).  Every spoiling keeps the list sorted."""
    import torch
    rows = list(GOOD)
    genome = random_letters(21, 30) + random_letters(22, 30)
    if what == 'alt_long':
        rows[5] = (30, 15, 1, 'ACGTACG')
    elif what == 'empty':
        rows[2] = (0, 20, 0, '')
    elif what == 'same':
        rows[2] = (0, 20, 2, genome[20:22])
    vs, _, _ = make_set(rows, [0, 30, 60])
    one = lambda v: torch.tensor([v], dtype=torch.int64, device=vs.var_off.device)            # noqa: E731
    if what == 'contig':
        vs.var_off[5:6] = one(33)
        return vs, genome, 5, pv.CONTIG
    if what == 'span':
        vs.var_pos[2:3] = one(29)
        vs.var_ndel[2] = 2
        return vs, genome, 2, pv.SPAN
    if what == 'before':
        vs.var_pos[0:1] = one(-1)
        return vs, genome, 0, pv.SPAN
    if what == 'ndel':
        vs.var_ndel[4] = -3
        return vs, genome, 4, pv.NDEL
    if what == 'alt_descends':
        vs.var_alt_off[6:7] = one(int(vs.var_alt_off[5]) - 1)
        return vs, genome, 5, pv.ALT
    if what == 'alt_outside':
        vs.var_alt_off[6:7] = one(vs.A + 2)
        return vs, genome, 5, pv.ALT
    return vs, genome, {'alt_long': 5, 'empty': 2, 'same': 2}[what], {'alt_long': pv.ALT, 'empty': pv.EMPTY, 'same': pv.SAME}[what]


@pytest.mark.parametrize("what", ['contig', 'span', 'before', 'ndel', 'alt_descends', 'alt_outside', 'alt_long', 'empty', 'same'])
def test_every_refusal_gives_its_status(what):
    """Each SLK_VARIANT_* case once, through the entries with a spoiled device array: the variant has its status and no candidate, its
    neighbours theirs, each as the model has it for the list without the spoiled entry."""
    need_gpu()
    vs, genome, bad, code = spoiled(what)
    windows = [(0, 0, 30, False), (30, 0, 30, True), (0, 1, 29, True), (30, 0, 30, False)]
    c = device_edits(genome, windows, vs, 3, 0)
    status = c.var_status.cpu().numpy()
    assert status[bad] == code and not np.delete(status, bad).any()
    rest = [v for i, v in enumerate(GOOD) if i != bad]
    want = pv.variant_edits(genome, [0, 30, 60], windows, rest, 3, 0, 0)
    renumber = np.array([i for i in range(len(GOOD)) if i != bad])
    assert np.array_equal(c.cand_off.cpu().numpy(), want["cand_off"])
    for name in ARRAYS:
        assert np.array_equal(getattr(c, name).cpu().numpy(), want[name]), name
    assert np.array_equal(c.cand_var.cpu().numpy(), renumber[want["cand_var"]])
    assert np.array_equal(c.cand_new.cpu().numpy()[:len(want["cand_new"])], want["cand_new"])
    assert c.ncand == 2 * (len(GOOD) - 1)


def test_host_wrapper_refuses_the_same_rows():
    need_gpu()
    from sloika_amd import genome, polish
    a, b = random_letters(21, 30), random_letters(22, 30)
    idx = genome.Index([("a", a), ("b", b)], k=8)
    good = [("a", 3, 2, ''), ("b", 2, 0, 'TT')]
    for row, word in ((("c", 3, 1, ''), "contig"), (("a", 29, 2, ''), "span"), (("a", -1, 0, 'A'), "span"), (("b", 11, -3, 'A'), "negative"),
                      (("b", 15, 1, 'ACGTACG'), "more letters"), (("a", 20, 0, ''), "nothing"), (("a", 20, 2, a[20:22]), "stand there")):
        with pytest.raises(ValueError) as e:
            polish.upload_variants(idx, good + [row], 3)
        assert "variant 2" in str(e.value) and word in str(e.value)
    vs = polish.upload_variants(idx, [("b", 2, 0, 'TT'), ("a", 3, 2, ''), (1, 2, 1, ''), ("a", 3, 0, 'G')], 3)
    assert vs.order.tolist() == [1, 3, 0, 2] and vs.rows() == [("b", 2, 0, 'TT'), ("a", 3, 2, ''), ("b", 2, 1, ''), ("a", 3, 0, 'G')]


# ---- 3: the sum ----------------------------------------------------------------------------------------------------------------------

def sum_case():
    """Five reads on both strands with staggered coverage of 9 variants: variant 2 is covered by read 0 alone, variant 5 by none."""
    rng = np.random.default_rng(11)
    score = -rng.uniform(200.0, 300.0, size=5)
    minus = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    cover = [range(0, 5), range(0, 2), range(3, 5), list(range(3, 5)) + list(range(6, 9)), range(6, 9)]
    cover = [[v for v in c if v != 2 or r == 0] for r, c in enumerate(cover)]
    read = np.array([r for r, c in enumerate(cover) for _ in c], dtype=np.int32)
    var = np.array([v for c in cover for v in c], dtype=np.int32)
    ll = score[read] + rng.normal(0.0, 3.0, size=len(read))
    ll[np.flatnonzero((var == 3) & (read == 2))] = -np.inf
    ll[np.flatnonzero((var == 7) & (read == 3))] = np.nan
    return score, minus, ll, read, var


def python_sum(score, minus, ll, read, var, V):
    t = [np.zeros(V), np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32), np.zeros((V, 2)), np.zeros((V, 2), dtype=np.int32),
         np.zeros((V, 2), dtype=np.int32)]
    for r in range(len(score)):                                      # read order, one float64 addition after the other
        for i in np.flatnonzero(read == r):
            v, k = int(var[i]), int(minus[r] != 0)
            if ll[i] != ll[i]:
                t[0][v] = np.nan
                t[3][v, k] = np.nan
            elif np.isfinite(ll[i]):
                d = ll[i] - score[r]
                t[0][v] = t[0][v] + d
                t[3][v, k] = t[3][v, k] + d
                t[1][v] += 1
                t[4][v, k] += 1
                t[2][v] += int(d > 0)
                t[5][v, k] += int(d > 0)
    return t


def tables_equal(got, want):
    got = [g.cpu().numpy() if hasattr(g, 'cpu') else g for g in got]
    for g, w in zip(got, want):
        if w.dtype == np.float64:
            assert np.array_equal(np.isnan(g), np.isnan(w)) and same_bits(np.nan_to_num(g, nan=-1.0), np.nan_to_num(w, nan=-1.0))
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w)
    return True


def test_sum_in_read_order():
    from sloika_amd import polish
    need_gpu()
    score, minus, ll, read, var = sum_case()
    V = 9
    want = python_sum(score, minus, ll, read, var, V)
    assert tables_equal(pv.sum_variant_gains(score, ll, read, var, minus, V), want)
    run = lambda sel, tables=None: polish.sum_variant_gains(dev(score), dev(ll[sel]), dev(read[sel]), dev(var[sel]), dev(minus), V, tables)   # noqa: E731
    everything = np.arange(len(ll))
    got = run(everything)
    assert tables_equal(got, want)
    gain, support, pro, gs, ss, ps = (t.cpu().numpy() for t in got)
    assert support[2] == 1 and ss[2].tolist() == [1, 0] and support[5] == 0 and gain[5] == 0.0 and not gs[5].any()
    assert support[3] == 2 and np.isfinite(gain[3])                 # the -inf of read 2 is not counted
    assert np.isnan(gain[7]) and np.isnan(gs[7, 1]) and not np.isnan(gs[7, 0]) and np.isnan(gain).sum() == 1 and np.isnan(gs).sum() == 1
    assert (pro <= support).all() and 0 < pro.sum() < support.sum() and np.array_equal(ss.sum(1), support) and np.array_equal(ps.sum(1), pro)
    # the candidates handed over in reversed read-block order
    rev = np.concatenate([np.flatnonzero(read == r) for r in range(4, -1, -1)])
    assert tables_equal(run(rev), want)
    # two launches that come in read order, adding into the tables of the first
    first = read < 2
    assert tables_equal(run(np.flatnonzero(~first), run(np.flatnonzero(first))), want)


# ---- 4: scores -----------------------------------------------------------------------------------------------------------------------

def called(sample):
    """The planted posteriors on the device, decoded by the real decoder."""
    from sloika_amd import decode
    post, steps = dev(sample["post"]), dev(sample["steps"])
    _, paths, lens, move_row, _, _ = decode.viterbi_marginals_batch(post, sample["k"], min_prob=MIN_PROB, lengths=steps)
    return post, steps, paths, lens, move_row


def test_scores_are_the_scoring_entry_bit_for_bit():
    """Nine reads on windows of fewer than 255 k-mers at W = 256 (lo all 0): every score and ll_edit of rescore_variants has the bits
    decode.rescore_edits_banded_batch returns for the read's rows, its window's string, the same centre line and the MODEL's triples."""
    need_gpu()
    from sloika_amd import decode, genome, polish
    s = pg.planted_genome(seed=4, windows=pg.SHORT_WINDOWS)
    k, draft = s["k"], s["draft"]
    post, steps, paths, lens, move_row = called(s)
    idx = genome.Index([("draft", draft)], k=14)
    res, strand, info, _, ops = idx.map_paths(paths, lens, k, ops=True)
    caller = random_variants(17, 0, 0, len(draft), 150, k) + [(0, p, nd, alt) for _, p, nd, alt in pv.repeat_variants(draft, [0, len(draft)], k)]
    caller = [v for v in caller if pv.variant_status(draft, [0, len(draft)], v, k) == pv.OK]
    got = polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k,
                                  [("draft", p, nd, alt) for _, p, nd, alt in caller], width=256)
    done = np.flatnonzero(got.status == polish.READ_DONE)
    assert done.tolist() == list(range(8)) + [9] and got.status[8] == polish.READ_UNMAPPED
    rows_sorted, order = pv.sort_variants(caller)
    w = polish.read_windows(paths, lens, move_row, steps, ops, strand, info, idx, k)
    center, score = w.center.cpu().numpy(), got.score.cpu().numpy()
    cand_read, cand_var, ll = got.cand_read.cpu().numpy(), got.cand_var.cpu().numpy(), got.ll_edit.cpu().numpy()
    compared = 0
    for r in done:
        r0, r1 = (int(v) for v in got.span[r])
        win = (0, int(got.window[r][0]), int(got.window[r][1]), strand[r] == '-')
        m = pv.variant_edits(draft, [0, len(draft)], [win], rows_sorted, k, 0, 2 * k)
        assert len(m["seq"]) < 255
        off = m["cand_new_off"]
        trip = [(int(a), int(d), m["cand_new"][off[i]:off[i + 1]]) for i, (a, d) in enumerate(zip(m["cand_start"], m["cand_ndel"]))]
        cen = center[w.center_off_host[r]:w.center_off_host[r] + r1 - r0 + 1]
        lo = decode.band_lo(cen, len(m["seq"]), 256)
        assert not bool(lo.any())
        rows = dev(np.ascontiguousarray(s["post"][r0:r1, r, :]))
        sc, le = decode.rescore_edits_banded_batch(rows, [m["seq"]], [decode.EditSet.from_list(trip)], [lo], 256, blank=0,
                                                   row_off=np.array([0, r1 - r0]))
        assert same_bits(sc.cpu().numpy().reshape(-1)[0], score[r]), r
        mine = cand_read == r
        assert np.array_equal(cand_var[mine], np.asarray(order)[m["cand_var"]])
        assert same_bits(np.asarray(le[0].cpu().numpy() if isinstance(le, (list, tuple)) else le.cpu().numpy()).reshape(-1), ll[mine]), r
        compared += int(mine.sum())
    assert compared == len(ll) and compared > 300


# ---- 5: the repeat proposer ----------------------------------------------------------------------------------------------------------

REPEAT_STRINGS = ["GCT" + "A" * 12 + "CGT", "GCT" + "AC" * 6 + "TGA", "T" + "ACG" * 4 + "TC", "G" + "ACGT" * 3 + "C", "AAAA", "ACACAC",
                  "GCTCACACAC", "ACACACGT", "TGACAC", "ACACTG", "GTACACNCACACTT", "NNNNNN", "TTACGACGANGACGACG"]


@pytest.mark.parametrize("klen", [3, 5])
def test_repeat_proposer_equals_the_model(klen):
    """A homopolymer of 12, (AC)x6, (ACG)x4, (ACGT)x3, AAAA (nothing at u = 2 or 4), tracts touching either contig end, two contigs
    whose strings would continue a tract across the boundary, an N inside a tract, random strings over AC and over ACGT -- each a
    contig of one index; a slice of a contig gives the slice of the whole; kmer_len 5 caps insertions at 4 letters."""
    need_gpu()
    from sloika_amd import genome, polish
    strings = REPEAT_STRINGS + [random_letters(31, 200, 'AC'), random_letters(32, 300), random_letters(33, 70, 'AC')]
    idx = genome.Index([("c%d" % i, s) for i, s in enumerate(strings)], k=8)
    packed, off = ''.join(strings), [int(v) for v in idx.offsets]
    name = dict((o, "c%d" % i) for i, o in enumerate(off[:-1]))
    want = pv.repeat_variants(packed, off, klen)
    got = polish.repeat_variants(idx, klen)
    assert got.rows() == [(name[o], p, nd, alt) for o, p, nd, alt in want] and len(want) > 150
    assert max(len(v[3]) for v in want) == min(pv.max_alt(klen), 4 if klen == 5 else 6)
    assert not [v for v in want if v[0] == off[4] and (len(v[3]) in (4,) or v[2] == 4)]          # AAAA: its unit is A alone
    assert np.array_equal(got.var_alt_off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(v[3]) for v in want])]))
    i = len(REPEAT_STRINGS)
    part = polish.repeat_variants(idx, klen, region=("c%d" % i, 40, 150))
    assert part.rows() == [(name[o], p, nd, alt) for o, p, nd, alt in want if o == off[i] and 40 <= p < 150] and len(part) > 10
    assert len(polish.repeat_variants(idx, klen, region=("c%d" % i, 40, 40))) == 0
    for kw in (dict(max_unit=2, max_change=1), dict(max_unit=3, max_change=4, min_copies=3)):
        assert polish.repeat_variants(idx, klen, **kw).rows() == [(name[o], p, nd, alt) for o, p, nd, alt in
                                                                  pv.repeat_variants(packed, off, klen, **kw)]
    # the proposals are a sorted variant set as they come: they go into the candidate kernels as they are
    c = device_edits(packed, [(off[1], 0, len(strings[1]), False), (off[1], 0, len(strings[1]), True)], got, klen, 0)
    m = pv.variant_edits(packed, off, [(off[1], 0, len(strings[1]), False), (off[1], 0, len(strings[1]), True)], want, klen, 0, 0)
    assert_edits_equal(c, m, np.arange(len(want)))


# ---- 6: planted repeats --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    need_gpu()
    from sloika_amd import genome
    s = pv.planted_repeats()
    call = called(s)
    idx = genome.Index([("draft", s["draft"])], k=14)
    keep = np.arange(len(s["texts"])) != 13
    res, strand, info, _, ops = idx.map_paths(call[2], call[3], s["k"], ops=True)
    fixes = [("draft",) + f for f in s["fixes"]]
    decoys = [("draft", 150, 0, 'ACAC'), ("draft", 170, 0, 'AC'), ("draft", 298, 0, 'AG')]
    return dict(sample=s, call=call, idx=idx, keep=keep, mapping=(res, strand, info, ops), variants=fixes + decoys)


def model_variants(text, k, call, host_post, mapping, keep, variants, width=256):
    """The CPU model on the device's mapping of the calls: tests/polish_genome_ref.py for windows and centre lines,
    tests/polish_variants_ref.py for candidates and the sum, tests/rescore_band_ref.evaluate (float64) for the scores.
    -> (the six tables in the caller's order, reads used, per variant the sum of max(1, |score|) over the reads counted)"""
    from tests import rescore_band_ref as rb
    res, strand, info, ops = mapping
    paths, lens, move_row, steps = (v.cpu().numpy() for v in call)
    qlen = ops.query_lengths()
    rows_sorted, order = pv.sort_variants(variants)
    score = np.full(len(steps), np.nan)
    reads, var, lls, used = [], [], [], []
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
        c = pv.variant_edits(text, [0, len(text)], [(0, win[0], win[1], strand[r] == '-')], rows_sorted, k, 0, 2 * k)
        off = c["cand_new_off"]
        trip = [(int(a), int(d), c["cand_new"][off[i]:off[i + 1]]) for i, (a, d) in enumerate(zip(c["cand_start"], c["cand_ndel"]))]
        sc, ll = rb.evaluate(host_post[span[0]:span[1], r, :], c["seq"], trip, rb.band_lo(cen, len(c["seq"]), width), width, 0, np.float64)
        score[r] = float(sc)
        reads += [r] * len(trip)
        var += [order[v] for v in c["cand_var"]]
        lls += [float(v) for v in ll]
    lls, reads, var = np.array(lls), np.array(reads, dtype=np.int32), np.array(var, dtype=np.int32)
    minus = np.array([x == '-' for x in strand], dtype=np.int32)
    tables = pv.sum_variant_gains(score, lls, reads, var, minus, len(variants))
    size = np.maximum(1.0, np.abs(score[reads]))
    scale = pv.sum_variant_gains(score, np.where(np.isfinite(lls), score[reads] + size, lls), reads, var, minus, len(variants))[0]
    return tables, used, scale


def test_planted_repeats(planted):
    """A draft that lacks one unit of (AC)x6, has a run of seven A two letters short and carries two letters too many, under 12 planted
    reads on both strands decoded and mapped by the real decoder and mapper.  The three true fixes and three decoys (the units one
    copy too many, the fix shifted out of its tract, another two-letter alt): every sign, and every gain to within 4 E_ref x the sum
    of max(1, |score|) over the reads counted (tests/test_gpu_polish_genome.py's bound, the same expression on E_REF), agrees with
    the float64 CPU model on the host posterior; the true fixes have support >= 3 and pro == support.  polish_genome(kinds=(),
    proposals='repeats') repairs the two repeat errors in one round, polish_genome with the explicit list returns the truth."""
    from sloika_amd import polish
    s, call, idx, keep, variants = planted["sample"], planted["call"], planted["idx"], planted["keep"], planted["variants"]
    post, steps, paths, lens, move_row = call
    res, strand, info, ops = planted["mapping"]
    k = s["k"]
    got = polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, variants, width=256, keep=keep)
    assert got.status.tolist() == [polish.READ_DONE] * 12 + [polish.READ_UNMAPPED, polish.READ_NOT_KEPT]
    tables, used, scale = model_variants(s["draft"], k, (paths, lens, move_row, steps), s["post"], (res, strand, info, ops), keep,
                                         [(0,) + v[1:] for v in variants])
    assert used == list(range(12))
    gain, support, pro, gs, ss, ps = (t.cpu().numpy() for t in (got.gain, got.support, got.pro, got.gain_strand, got.support_strand,
                                                                 got.pro_strand))
    for mine, model in ((support, tables[1]), (pro, tables[2]), (ss, tables[4]), (ps, tables[5])):
        assert np.array_equal(mine, model)
    assert np.isfinite(gain).all() and np.isfinite(tables[0]).all() and (support > 0).all()
    assert np.array_equal(np.sign(gain), np.sign(tables[0]))
    diff = np.abs(gain - tables[0])
    worst = float((diff / (E_REF * scale)).max())
    print("rescore_variants: gains %s (model %s), support %s, pro %s; largest |device - model| %.3g: %.3f of E_ref x (sum of max(1, |score|) "
          "over the reads counted)" % (np.round(gain, 3).tolist(), np.round(tables[0], 3).tolist(), support.tolist(), pro.tolist(),
                                      float(diff.max()), worst))
    assert worst <= 4.0
    for a, b in ((gs, tables[3]),):
        assert np.array_equal(np.sign(a), np.sign(b)) and (np.abs(a - b) <= 4.0 * E_REF * scale[:, None]).all()
    assert (support[:3] >= 3).all() and np.array_equal(pro[:3], support[:3]) and (gain[:3] > 0).all()
    assert (ss[:3] > 0).all()                                        # both strands saw every true fix
    reads, gains = got.read_gains(0)
    assert len(reads) == support[0] and (np.diff(reads) > 0).all() and (gains > 0).all()
    assert [r[:4] for r in got.top(3)] == sorted(variants[:3], key=lambda v: -gain[variants.index(v)])
    # the repeat family alone repairs the two repeat errors, in one round
    x = pv.REPEAT_EXTRA
    out, last, lastv = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, keep=keep, kinds=(), proposals='repeats')
    assert last is None and out[0].sequence == s["truth"][:x] + 'GT' + s["truth"][x:] and out[0].rounds == 1
    assert sorted(a[1:4] for a in out[0].applied) == [(150, 'var', (0, 'AC')), (298, 'var', (0, 'AA'))]
    assert all(a[0] == 0 and a[4] > 0 and a[5] >= 3 for a in out[0].applied)
    # the explicit list beside the single-letter cells returns the truth
    out, last, lastv = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, keep=keep, proposals=variants)
    assert out[0].sequence == s["truth"]
    assert sorted((a[1], a[3]) for a in out[0].applied if a[2] == 'var') == [(150, (0, 'AC')), (298, (0, 'AA')), (446, (2, ''))]
    assert last is not None and lastv is not None


def test_invariance(planted):
    """The nine tables do not depend on how the reads are cut into launches, on the unmapped read and the read failing keep being
    there at all, or on the caller's order of the variants."""
    import torch
    from sloika_amd import polish
    s, call, idx, keep = planted["sample"], planted["call"], planted["idx"], planted["keep"]
    post, steps, paths, lens, move_row = call
    res, strand, info, ops = planted["mapping"]
    k = s["k"]
    variants = planted["variants"] + [("draft", p, nd, alt) for _, p, nd, alt in pv.repeat_variants(s["draft"], [0, len(s["draft"])], k)]
    run = lambda v, **kw: polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, v, width=256, **kw)   # noqa: E731
    nine = lambda g: [t.cpu().numpy() for t in (g.gain, g.support, g.pro, g.gain_strand, g.support_strand, g.pro_strand)]             # noqa: E731
    whole = run(variants, keep=keep)
    want = nine(whole)
    assert want[1].max() >= 6 and np.isfinite(want[0]).all()
    nrow = (whole.span[:12, 1] - whole.span[:12, 0]).astype(np.int64)
    limit = int(16 * (nrow.max() + 1) * 257 * 5)                     # room for about five pairs: three launches or more
    assert tables_equal(nine(run(variants, keep=keep, workspace_limit=limit)), want)
    perm = np.random.RandomState(2).permutation(len(variants))
    shuffled = run([variants[i] for i in perm], keep=keep)
    assert tables_equal(nine(shuffled), [t[perm] for t in want])
    assert tables_equal(nine(run('repeats', keep=keep)), [t[6:] for t in want])
    # reads 12 (maps nowhere) and 13 (fails keep) absent altogether
    sub = idx.map_paths(paths[:12], lens[:12], k, ops=True)
    fewer = polish.rescore_variants(post[:, :12].contiguous(), steps[:12], paths[:12], lens[:12], move_row[:12], idx, sub[0], sub[1], sub[2],
                                    sub[4], k, variants, width=256)
    assert tables_equal(nine(fewer), want)
    both = nine(run(variants))                                       # read 13 spells read 0's window: it adds where read 0 scores
    assert (both[1] - want[1]).max() == 1 and (both[1] - want[1]).min() == 0


def test_unchanged_single_letter_path(planted):
    """rescore_genome and polish_genome(proposals=None) share their windows and bands with the new path now: the cells of the variants
    that are single-letter edits have the bits of rescore_variants, and polish_genome still returns two values."""
    from sloika_amd import polish
    s, call, idx, keep = planted["sample"], planted["call"], planted["idx"], planted["keep"]
    post, steps, paths, lens, move_row = call
    res, strand, info, ops = planted["mapping"]
    k = s["k"]
    cells = polish.rescore_genome(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256, keep=keep)
    singles = [("draft", 150, 1, ''), ("draft", 200, 1, 'ACGT'.replace(s["draft"][200], '')[0]), ("draft", 298, 0, 'A'), ("draft", 446, 1, '')]
    got = polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, singles, width=256, keep=keep)
    where = [cells.cell_of("draft", 150, 'del'), cells.cell_of("draft", 200, 'sub', singles[1][3]), cells.cell_of("draft", 298, 'ins', 'A'),
             cells.cell_of("draft", 446, 'del')]
    g, sp = cells.gain.cpu().numpy(), cells.support.cpu().numpy()
    assert same_bits(got.gain.cpu().numpy(), [g[p, q] for p, q in where])
    assert got.support.cpu().numpy().tolist() == [int(sp[p, q]) for p, q in where]
    out = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, keep=keep, max_rounds=1)
    assert len(out) == 2 and isinstance(out[1], polish.GenomeRescored)


# ---- 7: joins ------------------------------------------------------------------------------------------------------------------------

def test_variants_join():
    """The planted pileup of tests/pileup_cases.py, its reads as planted posteriors: polish_variants(rescore_variants(proposals()))
    gives the two-letter insertion, which the GenomeRescored join reports as None, a positive gain with support >= 3, and the
    single-letter rows the values of the GenomeRescored join to the same bits."""
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
    props = cons.proposals(polish.max_alt(k))
    assert len(props) < len(cons.variants())                         # the two deleted letters of the CA unit are one variant
    letters = polish.rescore_genome(post, steps_d, paths, lens, move_row, idx, res, strand, info, ops, k, width=256)
    got = polish.rescore_variants(post, steps_d, paths, lens, move_row, idx, res, strand, info, ops, k, props, width=256)
    old, new = cons.polish_variants(letters), cons.polish_variants(got)
    assert [v[:7] for v in new] == [v[:7] for v in old] and [v[-1] for v in new] == [v[-1] for v in old]
    longer = [(a, b) for a, b in zip(old, new) if a[2] == 'ins' and len(a[4]) == 2]
    assert len(longer) == 1 and longer[0][0][-3:] == (None, 0, False)
    assert longer[0][1][-3] > 0.0 and longer[0][1][-2] >= 3 and longer[0][1][-1] is False
    which = genome.proposals_of(cons.variants())[1]
    alone = [i for i, v in enumerate(old) if v[-1] and which.count(which[i]) == 1]
    assert len(alone) >= 3
    for i in alone:
        assert same_bits(new[i][-3], old[i][-3]) and new[i][-2] == old[i][-2] and old[i][-2] >= 3, old[i]
    merged = [i for i, v in enumerate(old) if which.count(which[i]) == 2]
    assert len(merged) == 2 and new[merged[0]][-3:] == new[merged[1]][-3:] and new[merged[0]][-3] > 0.0 and new[merged[0]][-2] >= 3


def test_basecaller_rescore_variants():
    """Two synthetic reads through a small built model, the genome a stretch of each read's own call: Basecaller.rescore_variants is
    polish.rescore_variants on the posterior, the calls and the mapping of the same reads, bit for bit; proposals= goes through
    Basecaller.polish_genome."""
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
    variants = [("a", 40, 2, ''), ("b", 30, 0, 'ACGT'), ("a", 60, 3, 'T')]
    got = bc.rescore_variants(reads, idx, variants, width=256)
    padded, ns = bc._padded_reads(reads, (0, 0), 0.0, None, "test")
    post, steps = bc._read_posteriors(padded, ns)
    res, strand, info, _, ops = idx.map_paths(paths, lens, 5, ops=True)
    want = polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, 5, variants, width=256, blank=0,
                                   min_prob=bc.min_prob)
    bits = lambda t: t.cpu().numpy().tobytes()                    # noqa: E731
    assert got.status.tolist() == want.status.tolist() and got.window.tolist() == want.window.tolist()
    for name in polish.VARIANT_TABLES + ("score", "var_status", "ll_edit", "cand_var", "cand_read"):
        assert bits(getattr(got, name)) == bits(getattr(want, name)), name
    assert got.variants.rows() == variants and got.var_status.cpu().numpy().tolist() == [0, 0, 0]
    out, last, lastv = bc.polish_genome(reads, idx, width=256, min_support=1, max_rounds=2, proposals='repeats')
    assert [(o.name, o.sequence) for o in out] == [("a", calls[0][20:144]), ("b", calls[1][10:94])] or any(o.applied for o in out)
    assert lastv.status.tolist() == last.status.tolist()
