"""Pileup and consensus on the device: csrc/pileup.hip through its three exports and through sloika_amd.genome, against the
plain-loop model of tests/pileup_ref.py (written from design/pileup.md section 1).  Every comparison is an integer or byte
equality.  Alignments are a few hundred columns at the most."""
import numpy as np
import pytest

from tests import pileup_cases
from tests import pileup_ref as R
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

M, X, I, D = R.MATCH, R.MISMATCH, R.INSERTION, R.DELETION
CANARY = 0xEE
EMPTY_ROW = [0] * 9


def fwd_pair(rs, fcodes, minus, t0, letter=None, qpad=(2, 3), rpad=(1, 2)):
    """A pair whose FORWARD view has the columns `fcodes`, as the device stores it -> (q, r, row, stored codes, minus, t0).
    letter(column) -> the column's letter (the query's, or the reference's in a deletion), or None: mostly A, so that gaps have
    somewhere to go."""
    Q, Rf = [], []
    for k, c in enumerate(fcodes):
        a = (letter(k) if letter else None) or "AAAC"[rs.randint(0, 4)]
        if c != D:
            Q.append(a)
        if c == M or c == D:
            Rf.append(a)
        elif c == X:
            Rf.append([x for x in "ACGTN" if x != a][rs.randint(0, 4)])
    Q, Rf = ''.join(Q), ''.join(Rf)
    pad = lambda n: ''.join("ACGT"[v] for v in rs.randint(0, 4, size=n))     # noqa: E731
    qc, rc, codes = (R.revcomp(Q).decode(), R.revcomp(Rf).decode(), list(fcodes)[::-1]) if minus else (Q, Rf, list(fcodes))
    q, r = pad(qpad[0]) + qc + pad(qpad[1]), pad(rpad[0]) + rc + pad(rpad[1])
    row = [1, qpad[0], qpad[0] + len(qc), rpad[0], rpad[0] + len(rc)] + [codes.count(k) for k in range(4)]
    return q, r, row, np.array(codes, dtype=np.uint8), bool(minus), int(t0)


def launch(pairs, G, genome, lo, hi, S, normalise=True, keep=None, tb=None, min_depth=3, tables=None, ops_off=None):
    """The three exports on one batch -> dict of host arrays.  tables: (counts, ins) device tensors to add to."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    B = len(pairs)
    ldq = max([len(p[0]) for p in pairs] + [1])
    qh = np.zeros((B, ldq), dtype=np.uint8)
    for b, p in enumerate(pairs):
        qh[b, :len(p[0])] = np.frombuffer(p[0].encode(), dtype=np.uint8)
    qlen = np.array([len(p[0]) for p in pairs], dtype=np.int32)
    rlen = np.array([len(p[1]) for p in pairs], dtype=np.int64)
    roff = np.concatenate(([0], np.cumsum(rlen))).astype(np.int64)
    rh = np.frombuffer((''.join(p[1] for p in pairs) + "ACGTACGT").encode(), dtype=np.uint8)
    rows = np.array([p[2] for p in pairs], dtype=np.int32).reshape(B, 9)
    if ops_off is None:
        ops_off = np.concatenate(([0], np.cumsum([len(p[3]) for p in pairs]))).astype(np.int64)
    codes = np.concatenate([np.asarray(p[3], dtype=np.uint8) for p in pairs] + [np.zeros(8, dtype=np.uint8)])
    keep = np.ones(B, dtype=np.uint8) if keep is None else np.asarray(keep, dtype=np.uint8)
    tb = np.zeros(B, dtype=np.int32) if tb is None else np.asarray(tb, dtype=np.int32)
    minus = np.array([int(p[4]) for p in pairs], dtype=np.int32)
    t0 = np.array([p[5] for p in pairs], dtype=np.int64)
    P = hi - lo
    d = {k: dev(v) for k, v in dict(q=qh, qlen=qlen, r=rh, roff=roff, rows=rows, ops=codes, off=ops_off, keep=keep, tb=tb, minus=minus,
                                    t0=t0, genome=np.frombuffer(genome.encode(), dtype=np.uint8)).items()}
    fcodes = torch.full((len(codes),), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((max(B, 1),), 99, dtype=torch.int32, device="cuda")
    counts, ins = tables if tables is not None else (torch.zeros((max(P, 1), 8), dtype=torch.int32, device="cuda"),
                                                     torch.zeros((max(P, 1), S, 5), dtype=torch.int32, device="cuda"))
    letters = torch.full((max(P, 1), 1 + S), CANARY, dtype=torch.uint8, device="cuda")
    nlet = torch.full((max(P, 1),), CANARY, dtype=torch.uint8, device="cuda")
    flags = torch.full((max(P, 1),), CANARY, dtype=torch.uint8, device="cuda")
    nbytes = int(ops_off[-1])
    _lib.check(L.slk_pileup_columns_u8(d['q'].data_ptr(), ldq, d['qlen'].data_ptr(), d['r'].data_ptr(), d['roff'].data_ptr(),
                                       d['rows'].data_ptr(), d['ops'].data_ptr(), d['off'].data_ptr(), nbytes, d['tb'].data_ptr(),
                                       d['minus'].data_ptr(), d['keep'].data_ptr(), d['t0'].data_ptr(), G, B, int(normalise),
                                       fcodes.data_ptr(), status.data_ptr(), stream()), "columns")
    _lib.check(L.slk_pileup_count_u8(d['q'].data_ptr(), ldq, d['qlen'].data_ptr(), d['roff'].data_ptr(), d['rows'].data_ptr(),
                                     fcodes.data_ptr(), d['off'].data_ptr(), nbytes, status.data_ptr(), d['minus'].data_ptr(),
                                     d['t0'].data_ptr(), G, B, lo, hi, S, counts.data_ptr(), ins.data_ptr(), stream()), "count")
    _lib.check(L.slk_pileup_call_u8(counts.data_ptr(), ins.data_ptr(), d['genome'].data_ptr(), G, lo, hi, S, min_depth,
                                    letters.data_ptr(), nlet.data_ptr(), flags.data_ptr(), stream()), "call")
    torch.cuda.synchronize()
    return {'fcodes': fcodes.cpu().numpy(), 'status': status.cpu().numpy()[:B], 'counts': counts.cpu().numpy()[:P],
            'ins': ins.cpu().numpy()[:P], 'letters': letters.cpu().numpy()[:P], 'nlet': nlet.cpu().numpy()[:P],
            'flags': flags.cpu().numpy()[:P], 'off': ops_off, 'tables': (counts, ins)}


def model(pairs, live, genome, lo, hi, S, normalise=True, min_depth=3):
    """What `launch` must return for the pairs `live` marks (the others add nothing and leave their slices alone)."""
    counts, ins, views = R.pile([p for p, ok in zip(pairs, live) if ok], lo, hi, S, normalise)
    _, parts, flags = R.consensus(counts, ins, genome, lo, min_depth)
    letters = np.zeros((hi - lo, 1 + S), dtype=np.uint8)
    for p, text in enumerate(parts):
        letters[p, :len(text)] = np.frombuffer(text, dtype=np.uint8)
    views = iter(views)
    return {'counts': np.array(counts, dtype=np.int32).reshape(hi - lo, 8), 'ins': np.array(ins, dtype=np.int32).reshape(hi - lo, S, 5),
            'letters': letters, 'nlet': np.array([len(t) for t in parts], dtype=np.uint8), 'flags': np.array(flags, dtype=np.uint8),
            'views': [np.array(next(views), dtype=np.uint8) if ok else None for ok in live]}


def compare(got, want, what=""):
    for b, view in enumerate(want['views']):
        have = got['fcodes'][got['off'][b]:got['off'][b + 1]]
        if view is None:
            assert (have == CANARY).all(), "%s: pair %d's slice of fcodes was written" % (what, b)
        else:
            assert have.tolist() == view.tolist(), "%s: pair %d's forward view" % (what, b)
    assert (got['fcodes'][got['off'][-1]:] == CANARY).all()
    for key in ('counts', 'ins', 'letters', 'nlet', 'flags'):
        assert np.array_equal(got[key], want[key]), "%s: %s" % (what, key)


def shapes(rs, S, minus_of):
    """The forward views the issue lists, as pairs; minus_of(k) -> strand of the k-th.  Positions start at 5, in a genome of 400."""
    A = lambda k: "A"                                                            # noqa: E731
    CA = lambda k: "C" if k == 0 else "A"                                        # noqa: E731
    rnd = lambda n, gaps=0.0: [int(v) for v in rs.choice([M, X, I, D], size=n, p=[0.8 - gaps, 0.2 - gaps, gaps, gaps])]   # noqa: E731
    views = [
        ([M], None), (rnd(63), None), (rnd(64, 0.05), None), (rnd(65, 0.08), None), (rnd(129, 0.08), None),
        ([M] * 5 + [I] + [M] * 5 + [I] * S + [X] * 5 + [I] * (S + 1) + [M] * 5, None),    # insertion runs of 1, S, S + 1
        ([M] * 62 + [I] * 5 + [M] * 10, None),                                   # a run from column 62 on
        ([M] * 61 + [D] * 6 + [M] * 8, None),                                    # a deletion run across column 64
        ([M] * 76 + [D] + [M] * 5, CA),                                          # a homopolymer: the gap crosses column 64 on its way
        ([M] * 30 + [I] * 100 + [M] * 5, CA),                                    # a run longer than a step, moved to column 1
        ([M] * 70 + [D] * 70 + [M] * 3, A),                                      # ... and one that stops at the alignment's start
        ([I] * 2 + [M] * 10, None),                                              # an insertion as the first column
        ([M] * 3 + [D] * 2 + [I] * 2 + [M] * 3 + [I] + [D] + [M] * 2, A),        # runs of both kinds that abut
    ]
    return [fwd_pair(rs, v, minus_of(k), 5 + 11 * k, letter) for k, (v, letter) in enumerate(views)]


def test_empty_batch():
    got = launch([], 50, "ACGTN" * 10, 0, 50, 4)
    want = model([], [], "ACGTN" * 10, 0, 50, 4)
    compare(got, want, "B = 0")
    assert (got['flags'] == R.LOW).all() and got['letters'][:, 0].tobytes() == b"ACGTN" * 10


@pytest.mark.parametrize("S,strands", [(1, "alternate"), (4, "plus"), (4, "minus"), (16, "alternate")])
def test_hand_made_codes_through_the_three_exports(S, strands):
    rs = np.random.RandomState(100 + S)
    G = 400
    genome = ''.join("ACGTN"[v] for v in rs.choice(5, size=G, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    minus_of = {"alternate": lambda k: k % 2 == 1, "plus": lambda k: False, "minus": lambda k: True}[strands]
    pairs = shapes(rs, S, minus_of)
    for normalise in (True, False):
        for lo, hi in ((0, G), (40, 150)):                                   # the second region cuts reads at either end
            got = launch(pairs, G, genome, lo, hi, S, normalise=normalise, min_depth=2)
            assert got['status'].tolist() == [0] * len(pairs)
            compare(got, model(pairs, [True] * len(pairs), genome, lo, hi, S, normalise, 2), "S=%d %s [%d, %d)" % (S, strands, lo, hi))
    moved = model(pairs, [True] * len(pairs), genome, 0, G, S, True)['views']
    still = model(pairs, [True] * len(pairs), genome, 0, G, S, False)['views']
    assert sum(a.tolist() != b.tolist() for a, b in zip(moved, still)) >= 5  # the shapes do exercise the normalisation


def test_one_pair_and_five_with_a_skipped_and_an_empty_one():
    rs = np.random.RandomState(7)
    G = 300
    genome = ''.join("ACGT"[v] for v in rs.randint(0, 4, size=G))
    rnd = lambda n: [int(v) for v in rs.choice([M, X, I, D], size=n, p=[0.7, 0.1, 0.1, 0.1])]     # noqa: E731
    one = [fwd_pair(rs, rnd(150), True, 20)]
    got = launch(one, G, genome, 0, G, 4, min_depth=1)
    assert got['status'].tolist() == [0]
    compare(got, model(one, [True], genome, 0, G, 4, True, 1), "B = 1")
    empty = ("ACGT", "ACG", EMPTY_ROW, np.zeros(0, dtype=np.uint8), False, 0)
    pairs = [fwd_pair(rs, rnd(100), False, 3), fwd_pair(rs, rnd(90), True, 30), empty, fwd_pair(rs, rnd(129), False, 60),
             fwd_pair(rs, rnd(64), True, 200)]
    got = launch(pairs, G, genome, 0, G, 4, keep=[1, 0, 1, 1, 1], tb=[0, 0, 1, 0, 0], min_depth=1)
    assert got['status'].tolist() == [0, 1, 1, 0, 0]
    compare(got, model(pairs, [True, False, False, True, True], genome, 0, G, 4, True, 1), "B = 5")
    # an alignment of no columns that the traceback calls done adds nothing either
    pairs[2] = ("ACGT", "ACG", [1, 2, 2, 1, 1, 0, 0, 0, 0], np.zeros(0, dtype=np.uint8), False, 10)
    got = launch(pairs, G, genome, 0, G, 4, min_depth=1)
    assert got['status'].tolist() == [0] * 5
    compare(got, model(pairs, [True] * 5, genome, 0, G, 4, True, 1), "B = 5, no columns")


def test_refusals_leave_their_neighbours_alone():
    rs = np.random.RandomState(8)
    G = 260
    genome = ''.join("ACGT"[v] for v in rs.randint(0, 4, size=G))
    rnd = lambda n: [int(v) for v in rs.choice([M, X, I, D], size=n, p=[0.7, 0.1, 0.1, 0.1])]     # noqa: E731
    pairs = [fwd_pair(rs, rnd(80), k % 2 == 1, 10 + 20 * k) for k in range(9)]
    want_status = [0] * 9

    def doctor(b, code, row=None, codes=None, t0=None):
        q, r, row0, codes0, minus, t00 = pairs[b]
        pairs[b] = (q, r, row0 if row is None else row, codes0 if codes is None else codes, minus, t00 if t0 is None else t0)
        want_status[b] = code

    bad = pairs[1][3].copy()
    bad[70] = 7
    doctor(1, R.BAD_CODE, codes=bad)
    row = list(pairs[3][2])
    row[5], row[6] = row[5] + 1, row[6] - 1                                  # the sums still hold; the codes say otherwise
    doctor(3, R.CODE_COUNT, row=row)
    doctor(4, R.POSITION, t0=G - (pairs[4][2][4] - pairs[4][2][3]) + 1)
    doctor(5, R.POSITION, t0=-1)
    row = list(pairs[6][2])
    row[2] = len(pairs[6][0]) + 1
    row[5] += 1
    doctor(6, R.BAD_SPAN, row=row)
    row = list(pairs[7][2])
    row[5], row[7] = row[5] + 1, row[7] - 1
    if row[7] < 0:
        row[5], row[7] = row[5] - 2, row[7] + 2
    doctor(7, R.BAD_SUM, row=row)
    got = launch(pairs, G, genome, 0, G, 4, min_depth=1)
    assert got['status'].tolist() == want_status
    assert [R.check_pair(p[2], p[3], len(p[0]), len(p[1]), p[5], G) for p in pairs] == want_status
    compare(got, model(pairs, [s == 0 for s in want_status], genome, 0, G, 4, True, 1), "refusals")
    # an ops slice that is not the column count long
    off = np.concatenate(([0], np.cumsum([len(p[3]) for p in pairs[:1]]))).astype(np.int64)
    off[1] += 1
    short = launch(pairs[:1], G, genome, 0, G, 4, ops_off=off)
    assert short['status'].tolist() == [R.OPS] and not short['counts'].any() and (short['fcodes'] == CANARY).all()


@pytest.fixture(scope="module")
def mapped():
    need_gpu()
    from sloika_amd import genome
    case = pileup_cases.planted()
    idx = genome.Index([(pileup_cases.CONTIG, case['genome'])], k=8, bin_width=512)      # every window is the whole contig
    res, strand, info, ops = idx.map(case['reads'], ops=True)
    g = case['genome']
    pairs = []
    for b, read in enumerate(case['reads']):
        ws, we = int(info['window_start'][b]), int(info['window_end'][b])
        minus = strand[b] == '-'
        w = R.revcomp(g[ws:we]).decode('ascii') if minus else g[ws:we]
        row = [int(v) for v in ops.rows[b]]
        pairs.append((read, w, row, ops.codes(b), minus, we - row[4] if minus else ws + row[3]))
    return {'case': case, 'idx': idx, 'map': (res, strand, info, ops), 'pairs': pairs}


def test_mapped_reads_to_consensus(mapped):
    from sloika_amd import genome
    case, idx, pairs = mapped['case'], mapped['idx'], mapped['pairs']
    res, strand, info, ops = mapped['map']
    G = len(case['genome'])
    assert strand.tolist() == case['strands'] and (ops.status == 0).all()
    pile = genome.Pileup(idx, max_ins=4)
    status = pile.add(res, strand, info, ops)
    assert status.tolist() == [0] * len(pairs)
    counts, ins, views = R.pile(pairs, 0, G, 4, True)
    assert np.array_equal(pile.counts(), np.array(counts, dtype=np.int32))
    assert np.array_equal(pile.insertions(), np.array(ins, dtype=np.int32).reshape(G, 4, 5))
    assert all(pile.columns(b).tolist() == views[b] for b in range(len(pairs)))
    cons = pile.consensus(min_depth=3)
    want, parts, flags = R.consensus(counts, ins, case['genome'], 0, 3)
    assert cons.sequences() == [(pileup_cases.CONTIG, want.decode('ascii'))]
    assert cons.flags.tolist() == flags
    assert cons.sequences()[0][1] == case['sample']
    got = cons.variants()
    assert got == R.variants(counts, ins, case['genome'], 0, [0, G], [pileup_cases.CONTIG])
    assert [v[:5] for v in got] == case['variants']
    s = cons.summary()
    covered = sum(1 for f in flags if not f & R.LOW)
    assert (s['covered'], s['substitutions'], s['deleted'], s['inserted']) == (covered, 1, 3, 3)
    assert s['identity'] == 1.0 - 7.0 / covered
    # without normalisation the two strands vote for different places
    raw, raw_cons = genome.pileup(idx, res, strand, info, ops, normalise=False)
    c2, i2, _ = R.pile(pairs, 0, G, 4, False)
    assert np.array_equal(raw.counts(), np.array(c2, dtype=np.int32))
    assert raw_cons.sequences()[0][1] == R.consensus(c2, i2, case['genome'], 0, 3)[0].decode('ascii') != case['sample']


def test_batches_regions_and_keep(mapped):
    from sloika_amd import genome
    case, idx = mapped['case'], mapped['idx']
    res, strand, info, ops = mapped['map']
    G, B = len(case['genome']), len(case['reads'])
    whole = genome.Pileup(idx, max_ins=3)
    whole.add(res, strand, info, ops)
    # two batches of reads, mapped on their own, one after the other
    halves = genome.Pileup(idx, max_ins=3)
    for lo, hi in ((0, B // 2), (B // 2, B)):
        part = idx.map(case['reads'][lo:hi], ops=True)
        assert halves.add(*part).tolist() == [0] * (hi - lo)
    assert np.array_equal(halves.counts(), whole.counts()) and np.array_equal(halves.insertions(), whole.insertions())
    # the same through keep=
    masks = genome.Pileup(idx, max_ins=3)
    first = np.arange(B) < B // 2
    assert masks.add(res, strand, info, ops, keep=first).tolist() == [0 if k else 1 for k in first]
    masks.add(res, strand, info, ops, keep=~first)
    assert np.array_equal(masks.counts(), whole.counts()) and np.array_equal(masks.insertions(), whole.insertions())
    for region in ((pileup_cases.CONTIG, 0, 100), (0, 95, 333), (pileup_cases.CONTIG, 300, G), (0, 17, 17)):
        part = genome.Pileup(idx, region=region, max_ins=3)
        part.add(res, strand, info, ops)
        assert np.array_equal(part.counts(), whole.counts()[region[1]:region[2]]), region
        assert np.array_equal(part.insertions(), whole.insertions()[region[1]:region[2]]), region
        text = part.consensus().sequences()
        assert text == ([(pileup_cases.CONTIG, ''.join(
            R.call(whole.counts()[p], whole.insertions()[p], ord(case['genome'][p]))[0].decode('ascii')
            for p in range(region[1], region[2])))] if region[2] > region[1] else [])
    none = genome.Pileup(idx)
    assert none.add(res, strand, info, ops, keep=np.zeros(B, dtype=bool)).tolist() == [1] * B
    assert not none.counts().any() and not none.insertions().any()
    assert none.consensus().sequences() == [(pileup_cases.CONTIG, case['genome'])]


def test_limits_and_refusals_by_name(mapped):
    from sloika_amd import genome
    idx = mapped['idx']
    res, strand, info, ops = mapped['map']
    with pytest.raises(ValueError, match="region="):
        genome.Pileup(idx, max_ins=16, memory_limit=1000)
    with pytest.raises(ValueError, match="max_ins"):
        genome.Pileup(idx, max_ins=17)
    with pytest.raises(ValueError, match="region="):
        genome.Pileup(idx, region=("nowhere", 0, 1))
    # a read whose window is said to lie elsewhere falls off the genome: refused by name, its neighbours piled
    moved = dict(info)
    moved['window_start'] = info['window_start'].copy()
    moved['window_end'] = info['window_end'].copy()
    b = int(np.flatnonzero(strand == '+')[0])
    moved['window_start'][b] += len(mapped['case']['genome'])
    pile = genome.Pileup(idx)
    status = pile.add(res, strand, moved, ops, names=["read%d" % k for k in range(len(res))])
    assert status[b] == -5 and (np.delete(status, b) == 0).all()
    with pytest.raises(ValueError, match="read%d .*inside the packed genome" % b):
        pile.columns(b)
    rest = genome.Pileup(idx)
    rest.add(res, strand, info, ops, keep=np.arange(len(res)) != b)
    assert np.array_equal(pile.counts(), rest.counts())
