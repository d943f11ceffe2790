"""The CPU model of csrc/polish_genome.hip (tests/polish_genome_ref.py) pinned with no GPU: its candidate triples are those of
polish.draft_edits (bio.single_letter_edits plus bio.edit_states on the spelled-out strings) on either strand, equal strings get
equal triples, and its centre line on a planted alignment is a valid band_lo input within 2 of the planted path."""
import numpy as np
import pytest

from sloika_amd import bio, polish
from tests import polish_genome_ref as pg


def random_string(seed, n):
    rng = np.random.RandomState(seed)
    return ''.join('ACGT'[v] for v in rng.randint(0, 4, n))


def strings():
    """name -> (genome, w0, w1): random strings, a homopolymer of 12, a dinucleotide repeat, a run touching the window's end."""
    a, b = random_string(1, 20), random_string(2, 17)
    return {
        "random40": (random_string(3, 52), 5, 45),
        "random9": (random_string(4, 30), 11, 20),
        "homopolymer12": (a + 'G' * 12 + b, 3, 46),
        "dinucleotide": (a + 'CA' * 9 + b, 2, 50),
        "run_at_end": (a + 'T' * 7 + b, 4, 27),
        "run_at_start": (a + 'T' * 7 + b, 20, 40),
        "all_one_letter": ('A' * 30, 3, 25),
    }


def in_margin(kind, pos, n, margin):
    return margin <= pos <= n - margin if kind == 'ins' else margin <= pos < n - margin


@pytest.mark.parametrize("klen", [3, 5])
@pytest.mark.parametrize("minus", [False, True])
@pytest.mark.parametrize("name", sorted(strings()))
def test_triples_are_draft_edits(name, minus, klen):
    genome, w0, w1 = strings()[name]
    for margin in (0, 2, 2 * klen):
        got = pg.letter_edits(genome, [(0, w0, w1, minus)], klen, 0, 7, margin)
        s = pg.window_string(genome, 0, w0, w1, minus)
        n = len(s)
        cols, rows, eset = polish.draft_edits(s, klen, bio.EDIT_KINDS, 'ACGT', 0, 4 ** klen + 1)
        keep = [i for i, r in enumerate(rows) if in_margin(r[0], r[1], n, margin)]
        assert len(keep) == len(got["cand_start"]) == got["cand_off"][1]
        assert np.array_equal(got["seq"], cols)
        assert np.array_equal(got["cand_start"], eset.start[keep])
        assert np.array_equal(got["cand_ndel"], eset.ndel[keep])
        for x, i in enumerate(keep):
            want = eset.new[eset.new_off[i]:eset.new_off[i + 1]]
            assert np.array_equal(got["cand_new"][got["cand_new_off"][x]:got["cand_new_off"][x + 1]], want), (rows[i][:3], x)
            assert len(want) <= klen + 1
            # the edit on the forward strand spells the same string
            p, kind, slot = pg.edit_of(got["cand_edit"][x])
            fwd = genome[w0:w1]
            if kind == 'sub':
                letter = [c for c in 'ACGT' if c != fwd[p - w0]][slot]
            else:
                letter = '' if kind == 'del' else 'ACGT'[slot - 4]
            spelled = bio.apply_letter_edits(fwd, [(kind, p - w0, letter)])
            assert (pg.revcomp(spelled) if minus else spelled) == rows[i][3]
            assert kind == rows[i][0]


@pytest.mark.parametrize("mask", range(8))
def test_every_kinds_subset(mask):
    genome, w0, w1 = strings()["homopolymer12"]
    kinds = tuple(k for k in bio.EDIT_KINDS if mask & pg.KIND_BITS[k])
    got = pg.letter_edits(genome, [(0, w0, w1, False)], 3, 0, mask, 0)
    _, rows, eset = polish.draft_edits(genome[w0:w1], 3, kinds, 'ACGT', 0, 65)
    assert np.array_equal(got["cand_start"], eset.start) and np.array_equal(got["cand_ndel"], eset.ndel)
    assert np.array_equal(got["cand_new"], eset.new) and np.array_equal(got["cand_new_off"], eset.new_off)


@pytest.mark.parametrize("name", sorted(strings()))
def test_equal_strings_equal_triples(name):
    genome, w0, w1 = strings()[name]
    for klen in (3, 5):
        s = genome[w0:w1]
        seen = {}
        for kind, u, c in pg.window_edits(s, klen, 7, 0):
            a, d, m = pg.triple(s, kind, u, c, klen)
            t = pg.edited(s, kind, u, c)
            trip = (a, d, tuple(pg.column(t[a + x:a + x + klen], 0) for x in range(m)))
            assert seen.setdefault(t, trip) == trip, (kind, u, c)
        assert len(seen) < len(pg.window_edits(s, klen, 7, 0))


def test_window_shorter_than_margin_or_kmer():
    genome = random_string(5, 30)
    assert pg.letter_edits(genome, [(0, 2, 11, False)], 3, 0, 7, 5)["cand_off"][1] == 0         # 9 letters, margin 5
    assert pg.letter_edits(genome, [(0, 2, 6, False)], 5, 0, 7, 0)["cand_off"][1] == 0          # 4 letters, no 5-mer
    one = pg.letter_edits(genome, [(0, 2, 7, False)], 5, 0, 7, 0)                               # 5 letters: no deletion leaves a 5-mer
    assert one["cand_off"][1] == 5 * 7 + 4


@pytest.mark.parametrize("minus", [False, True])
@pytest.mark.parametrize("klen", [3, 5])
def test_centre_line_of_a_planted_alignment(klen, minus):
    case = pg.planted_read(7, nwin=60, klen=klen, minus=minus)
    st, span, win, center = pg.run_planted(case)
    assert st == pg.DONE
    r0, r1 = span
    L = 60 - klen + 1
    assert len(center) == r1 - r0 + 1 and center[0] == 0 and center[-1] == L and (np.diff(center) >= 0).all()
    # clipped ends lie outside the scored rows: the rows of the first and last k-mers of the call
    mr = case["move_row"]
    assert r0 > mr[0] and r1 < case["nrow"]
    assert r0 == mr[case["row"][1]] and r1 == mr[case["row"][2] - klen + 1]
    for width in (8, 16, 256):
        lo = pg.band_lo(center, L, width)
        assert lo is not None and lo[0] == 0 and lo[-1] + width > L and (np.diff(lo) >= 0).all()
    worst = 0
    for i, want in enumerate(case["planted"]):
        if want is None or want < 1:
            continue
        t = mr[i] - r0 + 1                                       # the row index behind the row in which k-mer i is entered
        if 0 <= t <= r1 - r0:
            worst = max(worst, abs(int(center[t]) - want))
    assert worst <= 2
    w0, w1 = win
    rs, re, rlen = case["row"][3], case["row"][4], case["rlen"]
    assert (w0, w1) == ((case["wstart"] + rlen - re - case["coff"], case["wstart"] + rlen - rs - case["coff"]) if minus else
                        (case["wstart"] + rs - case["coff"], case["wstart"] + re - case["coff"]))


def test_whole_read_and_refusals():
    case = pg.planted_read(9, nwin=40, klen=3, whole=True)
    st, span, _, center = pg.run_planted(case)
    assert st == pg.DONE and span == (0, case["nrow"]) and center[-1] == 38
    bad = dict(case)
    assert pg.run_planted(case, ops_len=len(case["codes"]) + 1)[0] == pg.OPS
    codes = case["codes"].copy()
    codes[5] = 7
    assert pg.run_planted(case, codes=codes)[0] == pg.BAD_CODE
    mr = case["move_row"].copy()
    mr[10] = mr[9] - 1
    assert pg.run_planted(case, move_row=mr)[0] == pg.MOVE_ROW
    assert pg.run_planted(case, path=case["path"][:-1])[0] == pg.PATH
    assert pg.run_planted(case, center_cap=3)[0] == pg.CENTER
    few = case["move_row"] // 8
    assert pg.run_planted(case, move_row=few, nrow=int(few[-1]) + 1)[0] == pg.FEW_ROWS
    assert bad == case


def test_letter_triple_is_edit_states():
    rng = np.random.RandomState(0)
    for trial in range(60):
        k = (3, 5)[trial % 2]
        n = rng.randint(k, 30)
        s = ''.join('ACGT'[v] for v in rng.randint(0, (2, 4)[trial % 3 == 0], n))
        old = bio.seq_to_states(s, k)
        for kind, u, c in pg.window_edits(s, k, 7, 0):
            a, d, new = bio.edit_states(old, bio.seq_to_states(pg.edited(s, kind, u, c), k))
            assert polish.letter_triple(s, kind, u, c, k) == (a, d, tuple(int(v) for v in new)), (s, kind, u, c)


def test_planted_genome_maps_cleanly():
    """Before the device test relies on it: under the model of the seed stage (tests/genome_ref.py) every planted window gets its
    strand with many votes and no second locus on the draft, the unrelated read gets none, and every planted difference is covered
    by at least 4 reads and lies more than the margin from both ends of at least 3 of them."""
    from tests import genome_ref as gr
    s = pg.planted_genome()
    truth, draft = s["truth"], s["draft"]
    assert len(draft) == len(truth) == 600 and draft != truth
    assert truth[pg.SAMPLE_RUN[0]:pg.SAMPLE_RUN[1]] == 'AAAAA' and draft[300:305] == 'AAAAG'
    assert bio.apply_letter_edits(draft, [('sub', 150, truth[150]), ('ins', 302, 'A'), ('del', 449, '')]) == truth
    table = gr.occurrences([("draft", draft)], 14)
    for r, text in enumerate(s["texts"]):
        got = gr.choose_strand(gr.seed(table, text, 14, 256, 64), 3)
        if r == 12:
            assert got is None
            continue
        strand, row = got
        assert strand == ('+' if r % 2 == 0 or r == 13 else '-') and row[1] >= 100 and row[2] <= 2, (r, row)
    margin = 6
    for p in (pg.SAMPLE_SUB, pg.SAMPLE_RUN[0] + 2, pg.SAMPLE_INS):
        cover = [(a, b) for a, b in pg.SAMPLE_WINDOWS if a <= p < b]
        assert len(cover) >= 4 and sum(1 for a, b in cover if p - a > margin + 3 and b - p > margin + 3) >= 3


def test_sum_in_read_order():
    score = np.array([-10.0, -11.0, -12.5, -9.0, -8.0])
    pair = np.array([0, 0, 1, 2, 2, 3, 4, 4], dtype=np.int32)
    edit = np.array([8, 17, 8, 8, 17, 17, 8, 33], dtype=np.int64)
    ll = np.array([-9.1, -10.2, -10.7, -np.inf, np.nan, -8.3, -7.9, -7.5])
    gain, support = pg.sum_gains(score, ll, pair, edit, 1, 4)
    want = 0.0
    for l, r in ((-9.1, 0), (-10.7, 1), (-7.9, 4)):
        want = want + (l - score[r])
    assert gain[0, 0] == want and support[0, 0] == 3              # the -inf of read 2 is not counted
    assert np.isnan(gain[1, 1])                                    # the NaN of read 2
    assert gain[3, 1] == -7.5 - score[4] and support[3, 1] == 1
    assert gain[2, 5] == 0.0 and support[2, 5] == 0
