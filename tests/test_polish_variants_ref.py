"""The host half of variants on genome coordinates, with no GPU (design/polish_variants.md): polish.variant_triple against
bio.edit_states on the spelled-out strings and against polish.letter_triple; the plain-loop model of tests/polish_variants_ref.py against
itself where it has two ways to the same answer; genome.proposals_of / Consensus.proposals on hand-made rows (Consensus needs device
tensors to construct, so its pure host logic is exercised through a stub that has variants() alone); accept_genome_variants."""
import types

import numpy as np
import pytest

from sloika_amd import bio, genome, polish
from tests import polish_genome_ref as pg
from tests import polish_variants_ref as pv


def spelled(s, pos, ndel, alt, k):
    t = s[:pos] + alt + s[pos + ndel:]
    a, d, new = bio.edit_states(bio.seq_to_states(s, k), bio.seq_to_states(t, k))
    return a, d, tuple(int(v) for v in new)


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("letters", ["A", "AC", "ACGT"])
def test_variant_triple_is_edit_states(k, letters):
    """Random replacements: ref_len and alt up to 6 letters, strings short enough that tracts run to either end."""
    rng = np.random.RandomState(10 * k + len(letters))
    tried = 0
    for _ in range(1500):
        n = int(rng.randint(k, 4 * k))
        s = ''.join(letters[v] for v in rng.randint(0, len(letters), n))
        pos = int(rng.randint(0, n + 1))
        ndel = int(rng.randint(0, min(6, n - pos) + 1))
        alt = ''.join(letters[v] for v in rng.randint(0, len(letters), int(rng.randint(0, 7))))
        if ndel + len(alt) == 0 or n - ndel + len(alt) < k:
            continue
        got = polish.variant_triple(s, pos, ndel, alt, k)
        assert got == spelled(s, pos, ndel, alt, k), (s, pos, ndel, alt)
        assert len(got[2]) <= len(alt) + k - 1
        tried += 1
    assert tried > 1000


@pytest.mark.parametrize("k", [3, 5])
def test_variant_triple_on_tracts(k):
    """Tracts that run to either end of the string, an alt of the maximum length, the deletion of a whole tract."""
    cap = polish.max_alt(k)
    for s in ("AC" * 9, "A" * 14, "GT" + "AC" * 7, "AC" * 7 + "GT", "T" + "ACG" * 5 + "T"):
        n = len(s)
        for pos in range(n + 1):
            for ndel in range(0, n - pos + 1):
                for alt in ("", "A", "AC", "ACG", "ACAC", "ACGTACGT"[:cap]):
                    if ndel + len(alt) == 0 or n - ndel + len(alt) < k:
                        continue
                    assert polish.variant_triple(s, pos, ndel, alt, k) == spelled(s, pos, ndel, alt, k), (s, pos, ndel, alt)
    s = "GGT" + "AC" * 6 + "TTG"
    assert polish.variant_triple(s, 3, 12, "", 3) == spelled(s, 3, 12, "", 3)                # the whole tract goes
    assert len(polish.variant_triple("GATTACAGATTACA", 7, 0, "ACGTACGT"[:cap], k)[2]) <= polish.decode.rescore_max_new()


@pytest.mark.parametrize("k", [3, 5])
def test_variant_triple_is_letter_triple(k):
    for s in ("GATTTTACAGGCATA", "A" * 9, "ACACACACAC"):
        for kind, pos, letter, _ in bio.single_letter_edits(s):
            if kind == 'del' and len(s) - 1 < k:
                continue
            rep = (pos, 1, letter) if kind == 'sub' else (pos, 1, '') if kind == 'del' else (pos, 0, letter)
            assert polish.variant_triple(s, rep[0], rep[1], rep[2], k) == polish.letter_triple(s, kind, pos, letter, k), (s, kind, pos, letter)


def test_equal_strings_get_equal_triples():
    s = "GGT" + "AC" * 6 + "TTAAAAAAAG"
    for k in (3, 5):
        seen = {}
        for pos in range(len(s) + 1):
            for ndel, alt in ((2, ''), (0, 'AC'), (0, 'CA'), (0, 'AA'), (2, 'A'), (4, ''), (0, 'ACAC')):
                if pos + ndel > len(s):
                    continue
                t = s[:pos] + alt + s[pos + ndel:]
                if t == s:
                    continue
                trip = polish.variant_triple(s, pos, ndel, alt, k)
                assert seen.setdefault(t, trip) == trip, (pos, ndel, alt)
        assert len(seen) < 7 * len(s)                               # (strings were spelled more than once)


def test_model_triples_and_candidates():
    """The model's own pieces: its triple is bio.edit_states on k-mer lists of any letters, a '-' window sees the reverse complement of
    the variant, the far end of a variant decides, and the order within a '-' window descends."""
    g = "GGT" + "AC" * 6 + "TTANAAAAAG"
    for k in (3, 5):
        for (u, ndel, alt) in ((3, 2, ''), (5, 0, 'AC'), (15, 1, 'G')):
            a, d, kmers = pv.triple(g[:18], u, ndel, alt, k)
            new = tuple(int(v) for km in kmers for v in bio.seq_to_states(km, k))
            assert (a, d, new) == spelled(g[:18], u, ndel, alt, k)
    variants, order = pv.sort_variants([(0, 9, 2, ''), (0, 3, 0, 'AC'), (0, 3, 2, ''), (0, 20, 2, 'T'), (0, 21, 3, '')])
    assert order == [1, 2, 0, 3, 4]
    status = [pv.variant_status(g, [0, len(g)], v, 3) for v in variants]
    assert status == [0] * 5
    assert pv.window_candidates(variants, status, (0, 3, 22, False), 3, 0) == [0, 1, 2, 3]      # (21, 3) sticks out by two letters
    assert pv.window_candidates(variants, status, (0, 3, 24, True), 3, 0) == [4, 3, 2, 1, 0]
    assert pv.window_candidates(variants, status, (0, 3, 24, False), 3, 2) == [2, 3]
    assert pv.window_edit((0, 3, 24, True), variants[3]) == (2, 2, 'A')
    got = pv.variant_edits(g, [0, len(g)], [(0, 3, 24, True)], variants, 3, 0, 0)
    s = pg.revcomp(g[3:24])
    assert got["cand_var"].tolist() == [4, 3, 2, 1, 0] and -1 in got["cand_new"].tolist()        # the N beside (20, 2, 'T')
    for i, v in enumerate(got["cand_var"]):
        u, ndel, alt = pv.window_edit((0, 3, 24, True), variants[v])
        t = s[:u] + alt + s[u + ndel:]
        a, d = int(got["cand_start"][i]), int(got["cand_ndel"][i])
        new = got["cand_new"][got["cand_new_off"][i]:got["cand_new_off"][i + 1]].tolist()
        old = pg.window_columns(s, 3, 0)
        assert old[:a] + new + old[a + d:] == pg.window_columns(t, 3, 0)


def test_model_refusals():
    g, off = "ACGTACGTAC" + "GGGG", [0, 10, 14]
    assert pv.variant_status(g, off, (3, 0, 1, ''), 3) == pv.CONTIG
    assert pv.variant_status(g, off, (0, 9, 2, ''), 3) == pv.SPAN and pv.variant_status(g, off, (10, -1, 0, 'A'), 3) == pv.SPAN
    assert pv.variant_status(g, off, (0, 2, -1, 'A'), 3) == pv.NDEL
    assert pv.variant_status(g, off, (0, 2, 0, 'ACGTACG'), 3) == pv.ALT and pv.variant_status(g, off, (0, 2, 0, 'ACGTAC'), 3) == pv.OK
    assert pv.variant_status(g, off, (0, 2, 0, 'ACGTA'), 5) == pv.ALT and pv.variant_status(g, off, (0, 2, 0, 'ACGT'), 5) == pv.OK
    assert pv.variant_status(g, off, (0, 2, 0, ''), 3) == pv.EMPTY
    assert pv.variant_status(g, off, (0, 2, 2, 'GT'), 3) == pv.SAME
    assert pv.variant_status(g, off, (0, 10, 0, 'A'), 3) == pv.OK and pv.variant_status(g, off, (10, 0, 0, 'A'), 3) == pv.OK


def test_model_repeats():
    rows = lambda g, **kw: [(p, nd, alt) for _, p, nd, alt in pv.repeat_variants(g, [0, len(g)], kw.pop('k', 3), **kw)]     # noqa: E731
    assert rows("GCTACACACACACTGA") == [(3, 2, ''), (3, 4, ''), (3, 0, 'AC'), (3, 0, 'ACAC')]
    assert rows("TAAAAG") == [(1, 2, ''), (1, 0, 'AA')]                                        # never the single-letter ones
    assert rows("AAAA") == [(0, 2, ''), (0, 0, 'AA')]                                          # not at u = 2 or 4
    assert rows("CACGACGACGACGT", k=5) == [(1, 3, ''), (1, 6, ''), (1, 0, 'ACG')]               # kmer_len 5: at most 4 letters in
    assert rows("TACGTACGTACGTG", max_change=1) == [(0, 4, ''), (0, 0, 'TACG')]                 # leftmost: the unit is the one at the front
    assert rows("ACACNCACAC") == [(0, 2, ''), (0, 0, 'AC'), (0, 0, 'ACAC'), (5, 2, ''), (5, 0, 'CA'), (5, 0, 'CACA')]
    assert rows("GACACT", min_copies=3) == [] and rows("GACACACT", min_copies=3)[0] == (1, 2, '')
    two = pv.repeat_variants("TGACAC" + "ACACTG", [0, 6, 12], 3)
    assert [v[:3] for v in two if v[2]] == [(0, 2, 2), (6, 0, 2)]                              # a tract does not cross the boundary
    whole = pv.repeat_variants("GGTACACACACACTTGAAAAC", [0, 21], 3)
    assert pv.repeat_variants("GGTACACACACACTTGAAAAC", [0, 21], 3, lo=4, hi=21) == [v for v in whole if v[1] >= 4]


def test_model_sum():
    score = np.array([-10.0, -20.0, np.nan])
    ll = np.array([-9.0, -21.0, -8.0, -np.inf, -5.0])
    read, var, minus = np.array([0, 1, 0, 1, 2]), np.array([0, 0, 1, 1, 2]), np.array([0, 1, 0])
    gain, support, pro, gs, ss, ps = pv.sum_variant_gains(score, ll, read, var, minus, 4)
    assert gain[:2].tolist() == [0.0, 2.0] and np.isnan(gain[2]) and gain[3] == 0.0
    assert support.tolist() == [2, 1, 0, 0] and pro.tolist() == [1, 1, 0, 0]
    assert gs[0].tolist() == [1.0, -1.0] and ss[0].tolist() == [1, 1] and ps[0].tolist() == [1, 0] and np.isnan(gs[2, 0]) and gs[2, 1] == 0.0


ROWS = [("c", 5, 'sub', 'A', 'G', 30, 25), ("c", 9, 'del', 'A', '', 30, 20), ("c", 10, 'del', 'A', '', 30, 21), ("c", 11, 'del', 'C', '', 30, 19),
        ("c", 13, 'del', 'T', '', 28, 18), ("c", 13, 'ins', '', 'GT', 28, 17), ("c", 14, 'del', 'T', '', 28, 18),
        ("c", 20, 'ins', '', 'A', 31, 22), ("c", 29, 'del', 'G', '', 31, 22), ("d", 30, 'del', 'G', '', 12, 9), ("d", 40, 'ins', '', 'ACGTA', 9, 8)]


def test_proposals_of_hand_made_rows():
    want = [("c", 5, 1, 'G'), ("c", 9, 3, ''), ("c", 13, 1, ''), ("c", 14, 0, 'GT'), ("c", 14, 1, ''), ("c", 21, 0, 'A'), ("c", 29, 1, ''),
            ("d", 30, 1, ''), ("d", 41, 0, 'ACGTA')]
    got, which = genome.proposals_of(ROWS)
    assert got == want and which == [0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8]
    stub = types.SimpleNamespace(variants=lambda: ROWS)               # (a Consensus holds device tensors: the host logic alone)
    assert genome.Consensus.proposals(stub) == want
    got, which = genome.proposals_of(ROWS, max_alt=4)
    assert got == want[:-1] and which[-1] is None and which[:-1] == [0, 1, 1, 1, 2, 3, 4, 5, 6, 7]
    assert genome.Consensus.proposals(stub, polish.max_alt(5)) == want[:-1]
    assert genome.proposals_of([]) == ([], [])


def test_accept_over_cells_and_variants():
    text = {"c": "GGTACACACACTTGCATTAGGCATCAAAAAGTCCA"}
    k = 3
    cells = [("c", 14, 'sub', 'T', 5.0, 4), ("c", 16, 'del', '', 3.0, 4), ("c", 30, 'ins', 'G', 1.0, 3)]
    variants = [("c", 3, 2, '', 9.0, 5, 5), ("c", 5, 2, '', 8.5, 5, 5), ("c", 9, 0, 'AC', 2.0, 3, 3), ("c", 25, 2, '', 4.0, 3, 3),
                ("c", 30, 0, 'G', 0.5, 3, 3)]
    taken = polish.accept_genome_variants(cells, variants, text, k)
    assert taken[0] == ("c", 3, 'var', (2, ''), 9.0, 5)                # (5, 2, '') spells the same string: passed over
    assert ("c", 5, 'var', (2, ''), 8.5, 5) not in taken
    assert ("c", 14, 'sub', 'T', 5.0, 4) in taken                     # 14 - 4 >= 3 from the deletion's last letter
    assert ("c", 16, 'del', '', 3.0, 4) not in taken                  # two letters from the substitution
    assert ("c", 25, 'var', (2, ''), 4.0, 3) in taken
    assert ("c", 9, 'var', (0, 'AC'), 2.0, 3) in taken                # 9 - 4 >= 3, 14 - 9 >= 3
    assert ("c", 30, 'ins', 'G', 1.0, 3) in taken and len(taken) == 5  # 30 - 26 >= 3; the same insertion as a variant is a duplicate
    # for cells alone it is accept_genome_edits
    more = cells + [("c", 17, 'sub', 'C', 2.5, 2), ("c", 26, 'del', '', 0.7, 2), ("c", 28, 'del', '', 0.6, 2)]
    assert polish.accept_genome_variants(more, [], text, k) == polish.accept_genome_edits(more, text, k)


def test_upload_refusals_name_the_row():
    """upload_variants refuses on the host what the kernel refuses on the device; none of it needs one."""
    class Ix(object):
        names, lengths, offsets = ["a", "b"], [10, 4], np.array([0, 10, 14])

        class genome(object):
            device = None

            @staticmethod
            def cpu():
                return types.SimpleNamespace(numpy=lambda: np.frombuffer(b"ACGTACGTACGGGG", dtype=np.uint8))
    good = ("a", 2, 0, "AC")
    for row, word in ((("z", 0, 1, ''), "contig"), ((2, 0, 1, ''), "contig"), (("a", 9, 2, ''), "span"), (("b", -1, 0, 'A'), "span"),
                      (("a", 2, -1, 'A'), "negative"), (("a", 2, 0, 'ACGTACG'), "more letters"), (("a", 2, 0, 'AN'), "none of"),
                      (("a", 2, 0, ''), "nothing"), (("a", 2, 2, 'GT'), "stand there")):
        with pytest.raises(ValueError) as e:
            polish.upload_variants(Ix, [good, row], 3)
        assert "variant 1" in str(e.value) and word in str(e.value), (row, str(e.value))
    with pytest.raises(ValueError):
        polish.upload_variants(Ix, [("a", 2, 0, 'ACGTA')], 5)
