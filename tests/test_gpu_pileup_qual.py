"""The quality-weighted pileup on the device: slk_pileup_count_qual_u8 and slk_pileup_call_qual_u8 through the C ABI and through
sloika_amd.genome, against the plain-loop model of tests/pileup_qual_ref.py (written from design/pileup.md section 9).  Every
comparison is an integer or byte equality.  Alignments are a few hundred columns at the most."""
import numpy as np
import pytest

from tests import align_cases, pileup_qual_cases
from tests import pileup_qual_ref as Q
from tests import pileup_ref as R
from tests import test_gpu_pileup as T
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

M, X, I, D = R.MATCH, R.MISMATCH, R.INSERTION, R.DELETION
CANARY = T.CANARY
ONES = np.ones(256, dtype=np.uint8)


def with_quals(rs, pairs):
    """Random quality bytes 0..255 for every letter of every pair's query -> pairs of seven."""
    return [p + (rs.randint(0, 256, size=len(p[0])).astype(np.uint8),) for p in pairs]


def launch(pairs, G, genome, lo, hi, S, weights, normalise=True, min_depth=3, qmax=60):
    """Columns, then BOTH count kernels on the same columns (each into tables of its own), then both call kernels -> dict of host
    arrays; the plain kernels' results under 'plain_*'."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    B = len(pairs)
    ldq = max([len(p[0]) for p in pairs] + [1])
    qh, vh = np.zeros((B, ldq), dtype=np.uint8), np.zeros((B, ldq), dtype=np.uint8)
    for b, p in enumerate(pairs):
        qh[b, :len(p[0])] = np.frombuffer(p[0].encode(), dtype=np.uint8)
        vh[b, :len(p[0])] = p[6]
    qlen = np.array([len(p[0]) for p in pairs], dtype=np.int32)
    rlen = np.array([len(p[1]) for p in pairs], dtype=np.int64)
    roff = np.concatenate(([0], np.cumsum(rlen))).astype(np.int64)
    rh = np.frombuffer((''.join(p[1] for p in pairs) + "ACGTACGT").encode(), dtype=np.uint8)
    rows = np.array([p[2] for p in pairs], dtype=np.int32).reshape(B, 9)
    ops_off = np.concatenate(([0], np.cumsum([len(p[3]) for p in pairs]))).astype(np.int64)
    codes = np.concatenate([np.asarray(p[3], dtype=np.uint8) for p in pairs] + [np.zeros(8, dtype=np.uint8)])
    minus = np.array([int(p[4]) for p in pairs], dtype=np.int32)
    t0 = np.array([p[5] for p in pairs], dtype=np.int64)
    P = hi - lo
    d = {k: dev(v) for k, v in dict(q=qh, qual=vh, qlen=qlen, r=rh, roff=roff, rows=rows, ops=codes, off=ops_off,
                                    keep=np.ones(B, dtype=np.uint8), tb=np.zeros(B, dtype=np.int32), minus=minus, t0=t0,
                                    genome=np.frombuffer(genome.encode(), dtype=np.uint8),
                                    weights=np.asarray(weights, dtype=np.uint8)).items()}
    fcodes = torch.full((len(codes),), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((max(B, 1),), 99, dtype=torch.int32, device="cuda")
    n = max(P, 1)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")          # noqa: E731
    counts, ins, wcounts, wins, pcounts, pins = zeros(n, 8), zeros(n, S, 5), zeros(n, 8), zeros(n, S, 5), zeros(n, 8), zeros(n, S, 5)
    out = {k: torch.full(shape, CANARY, dtype=torch.uint8, device="cuda")
           for k, shape in dict(letters=(n, 1 + S), nlet=(n,), flags=(n,), letq=(n, 1 + S), posq=(n,), plain_letters=(n, 1 + S),
                                plain_nlet=(n,), plain_flags=(n,)).items()}
    nbytes = int(ops_off[-1])
    _lib.check(L.slk_pileup_columns_u8(d['q'].data_ptr(), ldq, d['qlen'].data_ptr(), d['r'].data_ptr(), d['roff'].data_ptr(),
                                       d['rows'].data_ptr(), d['ops'].data_ptr(), d['off'].data_ptr(), nbytes, d['tb'].data_ptr(),
                                       d['minus'].data_ptr(), d['keep'].data_ptr(), d['t0'].data_ptr(), G, B, int(normalise),
                                       fcodes.data_ptr(), status.data_ptr(), stream()), "columns")
    _lib.check(L.slk_pileup_count_u8(d['q'].data_ptr(), ldq, d['qlen'].data_ptr(), d['roff'].data_ptr(), d['rows'].data_ptr(),
                                     fcodes.data_ptr(), d['off'].data_ptr(), nbytes, status.data_ptr(), d['minus'].data_ptr(),
                                     d['t0'].data_ptr(), G, B, lo, hi, S, pcounts.data_ptr(), pins.data_ptr(), stream()), "count")
    _lib.check(L.slk_pileup_count_qual_u8(d['q'].data_ptr(), ldq, d['qlen'].data_ptr(), d['qual'].data_ptr(), d['roff'].data_ptr(),
                                          d['rows'].data_ptr(), fcodes.data_ptr(), d['off'].data_ptr(), nbytes, status.data_ptr(),
                                          d['minus'].data_ptr(), d['t0'].data_ptr(), G, B, lo, hi, S, d['weights'].data_ptr(),
                                          counts.data_ptr(), ins.data_ptr(), wcounts.data_ptr(), wins.data_ptr(), stream()),
               "count_qual")
    _lib.check(L.slk_pileup_call_u8(pcounts.data_ptr(), pins.data_ptr(), d['genome'].data_ptr(), G, lo, hi, S, min_depth,
                                    out['plain_letters'].data_ptr(), out['plain_nlet'].data_ptr(), out['plain_flags'].data_ptr(),
                                    stream()), "call")
    _lib.check(L.slk_pileup_call_qual_u8(counts.data_ptr(), ins.data_ptr(), wcounts.data_ptr(), wins.data_ptr(),
                                         d['genome'].data_ptr(), G, lo, hi, S, min_depth, qmax, out['letters'].data_ptr(),
                                         out['nlet'].data_ptr(), out['flags'].data_ptr(), out['letq'].data_ptr(),
                                         out['posq'].data_ptr(), stream()), "call_qual")
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy()[:P] for k, v in out.items()}
    got.update(status=status.cpu().numpy()[:B], counts=counts.cpu().numpy()[:P], ins=ins.cpu().numpy()[:P],
               wcounts=wcounts.cpu().numpy()[:P], wins=wins.cpu().numpy()[:P], plain_counts=pcounts.cpu().numpy()[:P],
               plain_ins=pins.cpu().numpy()[:P])
    return got


def call_arrays(counts, wcounts, wins, genome, lo, S, min_depth, qmax):
    """The model's weighted call of every position as the arrays slk_pileup_call_qual_u8 writes."""
    P = len(counts)
    _, parts, flags, quals, posq = Q.consensus(counts, wcounts, wins, genome, lo, min_depth, qmax)
    letters, letq = np.zeros((P, 1 + S), dtype=np.uint8), np.zeros((P, 1 + S), dtype=np.uint8)
    for p, (text, lq) in enumerate(zip(parts, quals)):
        letters[p, :len(text)] = np.frombuffer(text, dtype=np.uint8)
        letq[p, :len(lq)] = lq
    return {'letters': letters, 'letq': letq, 'nlet': np.array([len(t) for t in parts], dtype=np.uint8),
            'flags': np.array(flags, dtype=np.uint8), 'posq': np.array(posq, dtype=np.uint8)}


def model(pairs, genome, lo, hi, S, weights, normalise=True, min_depth=3, qmax=60):
    P = hi - lo
    counts, ins, wcounts, wins, _ = Q.pile(pairs, lo, hi, S, [int(w) for w in weights], normalise)
    want = call_arrays(counts, wcounts, wins, genome, lo, S, min_depth, qmax)
    want.update(counts=np.array(counts, dtype=np.int32).reshape(P, 8), ins=np.array(ins, dtype=np.int32).reshape(P, S, 5),
                wcounts=np.array(wcounts, dtype=np.int32).reshape(P, 8), wins=np.array(wins, dtype=np.int32).reshape(P, S, 5))
    return want


def compare(got, want, what):
    for key in ('counts', 'ins', 'wcounts', 'wins', 'letters', 'nlet', 'flags', 'letq', 'posq'):
        assert np.array_equal(got[key], want[key]), "%s: %s" % (what, key)
    assert np.array_equal(got['counts'], got['plain_counts']) and np.array_equal(got['ins'], got['plain_ins']), what + ": plain tables"


# ---- 1, 2. the hand-made forward views --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,strands", [(1, "alternate"), (4, "plus"), (4, "minus"), (16, "alternate")])
def test_hand_made_views_four_tables_and_the_weighted_call(S, strands):
    rs = np.random.RandomState(200 + S)
    G = 400
    genome = ''.join("ACGTN"[v] for v in rs.choice(5, size=G, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    minus_of = {"alternate": lambda k: k % 2 == 1, "plus": lambda k: False, "minus": lambda k: True}[strands]
    pairs = with_quals(rs, T.shapes(rs, S, minus_of))
    weights = Q.weights_table(5, 60)
    for normalise in (True, False):
        for lo, hi in ((0, G), (40, 150)):
            got = launch(pairs, G, genome, lo, hi, S, weights, normalise=normalise, min_depth=2)
            assert got['status'].tolist() == [0] * len(pairs)
            compare(got, model(pairs, genome, lo, hi, S, weights, normalise, 2), "S=%d %s [%d, %d)" % (S, strands, lo, hi))
    # a table of the caller's own: every byte is an index, weights up to 255
    own = rs.randint(0, 256, size=256).astype(np.uint8)
    got = launch(pairs, G, genome, 0, G, S, own, min_depth=1, qmax=93)
    compare(got, model(pairs, genome, 0, G, S, own, True, 1, 93), "S=%d %s own table" % (S, strands))


@pytest.mark.parametrize("S", [1, 4, 16])
def test_all_ones_weights_are_the_plain_count_and_call(S):
    rs = np.random.RandomState(300 + S)
    G = 400
    genome = ''.join("ACGTN"[v] for v in rs.choice(5, size=G, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    pairs = with_quals(rs, T.shapes(rs, S, lambda k: k % 2 == 1))
    assert all(p[2][2] > p[2][1] for p in pairs)                 # every alignment has a query letter
    for lo, hi in ((0, G), (40, 150)):
        got = launch(pairs, G, genome, lo, hi, S, ONES, min_depth=2)
        assert got['counts'].any() and got['ins'].any()
        assert np.array_equal(got['wcounts'], got['counts']) and np.array_equal(got['wins'], got['ins'])
        assert np.array_equal(got['counts'], got['plain_counts']) and np.array_equal(got['ins'], got['plain_ins'])
        for key in ('letters', 'nlet', 'flags'):
            assert np.array_equal(got[key], got['plain_' + key]), key


# ---- 3. the call kernel alone ------------------------------------------------------------------------------------------------------------

def call_alone(counts, ins, wcounts, wins, genome, S, min_depth=3, qmax=60, pad=7):
    """slk_pileup_call_qual_u8 on host tables of P positions; the outputs have `pad` canaried positions behind them."""
    torch = need_gpu()
    from sloika_amd import _lib
    P = len(counts)
    t = [dev(np.asarray(a, dtype=np.int32).reshape(shape)) for a, shape in
         ((counts, (P, 8)), (ins, (P, S, 5)), (wcounts, (P, 8)), (wins, (P, S, 5)))]
    g = dev(np.frombuffer(genome.encode(), dtype=np.uint8))
    out = {k: torch.full((P + pad,) + tail, CANARY, dtype=torch.uint8, device="cuda")
           for k, tail in dict(letters=(1 + S,), nlet=(), flags=(), letq=(1 + S,), posq=()).items()}
    _lib.check(_lib.lib().slk_pileup_call_qual_u8(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), g.data_ptr(),
                                                  len(genome), 0, P, S, min_depth, qmax, out['letters'].data_ptr(),
                                                  out['nlet'].data_ptr(), out['flags'].data_ptr(), out['letq'].data_ptr(),
                                                  out['posq'].data_ptr(), stream()), "call_qual")
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert (v[P:] == CANARY).all(), "%s written past P" % k
    return {k: v[:P] for k, v in host.items()}


#: hand-made positions: (counts row, wcounts row, wins rows for S = 2, reference letter), the cases of tests/test_pileup_qual_host.py
BIG = 1 << 30
HAND = [
    ([5, 1, 0, 0, 0, 0, 0, 6], [15, 30, 0, 0, 0, 0, 0, 45], None, 'A'),
    ([1, 1, 0, 0, 0, 0, 0, 2], [40, 0, 0, 0, 0, 0, 0, 40], None, 'N'),                    # LOW by depth
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 0, 0, 0, 9, 0, 0, 9], None, 'C'),                      # zero weights under sufficient depth
    ([6, 0, 0, 0, 0, 0, 2, 6], [0] * 8, [[5, 0, 0, 0, 0], [0] * 5], 'T'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [20, 0, 0, 20, 0, 20, 0, 60], None, 'T'),                  # ties
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 20, 0, 20, 0, 20, 0, 60], None, 'A'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 0, 20, 0, 0, 20, 0, 60], None, 'G'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 0, 20, 0, 0, 20, 0, 60], None, 'A'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [7, 7, 0, 0, 0, 7, 0, 21], None, 'N'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 0, 0, 5, 0, 30, 0, 35], None, 'T'),                    # the deletion wins
    ([6, 0, 0, 0, 0, 0, 0, 6], [0, 0, 0, 0, 0, 30, 0, 30], None, 'N'),
    ([6, 0, 0, 0, 0, 0, 0, 6], [200, 10, 0, 0, 0, 0, 0, 210], None, 'A'),                 # posq capped
    ([6, 0, 0, 0, 0, 0, 0, 6], [50, 10, 0, 0, 35, 0, 0, 95], None, 'A'),                  # W_next from entry 4
    ([6, 0, 0, 0, 0, 0, 0, 6], [50, 10, 0, 0, 80, 0, 0, 140], None, 'A'),
    ([6, 0, 0, 0, 0, 0, 3, 6], [100, 0, 0, 0, 0, 0, 50, 100], [[0, 0, 50, 0, 0], [0] * 5], 'A'),
    ([6, 0, 0, 0, 0, 0, 3, 6], [100, 0, 0, 0, 0, 0, 51, 100], [[0, 0, 51, 0, 0], [0] * 5], 'A'),
    ([6, 0, 0, 0, 0, 0, 3, 6], [100, 0, 0, 0, 0, 0, 70, 100], [[0, 30, 30, 0, 10], [0] * 5], 'A'),   # quality clamped at 0
    ([6, 0, 0, 0, 0, 0, 3, 6], [100, 0, 0, 0, 0, 0, 90, 100], [[0, 0, 0, 90, 0], [0, 40, 0, 0, 0]], 'A'),   # stop at the first failing k
    ([6, 0, 0, 0, 0, 0, 3, 6], [100, 0, 0, 0, 0, 0, 90, 100], [[0, 0, 0, 0, 90], [0, 0, 0, 90, 0]], 'A'),
    ([0, 0, 0, 0, 0, 6, 3, 6], [0, 0, 0, 0, 0, 100, 80, 100], [[0, 80, 0, 0, 0], [0] * 5], 'A'),
    ([6, 0, 0, 0, 0, 0, 6, 6], [BIG, 0, 0, 0, 0, 0, BIG, BIG + 5], [[BIG, 0, 0, 0, 0], [BIG - 1, 0, 0, 0, BIG]], 'A'),   # 64-bit products
    ([6, 0, 0, 0, 0, 0, 6, 6], [BIG, BIG - 3, 0, 0, 0, 0, BIG, 2 * BIG - 1], [[BIG - 1, 1, 0, 0, 0], [0] * 5], 'C'),
]


@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_call_kernel_alone_on_hand_made_tables(P):
    S = 2
    rs = np.random.RandomState(P)
    rows = [HAND[(k + P) % len(HAND)] for k in range(P)]
    counts, wcounts = [r[0] for r in rows], [r[1] for r in rows]
    wins = [r[2] if r[2] is not None else [[0] * 5] * S for r in rows]
    ins = [[[int(v > 0) for v in slot] for slot in w] for w in wins]
    genome = ''.join(r[3] for r in rows)
    for qmax in (60, 93, 1):
        got = call_alone(counts, ins, wcounts, wins, genome, S, 3, qmax)
        want = call_arrays(counts, wcounts, wins, genome, 0, S, 3, qmax)
        for key in want:
            assert np.array_equal(got[key], want[key]), "P=%d qmax=%d: %s" % (P, qmax, key)
    if P >= len(HAND):                                           # every hand-made case took part, and they do what they are there for
        assert (want['flags'] & R.LOW).any() and (want['flags'] & R.INSERTED).any() and (want['nlet'] == 0).any()
    # random tables besides: weights up to 2^30 in every entry
    rc = rs.randint(0, 8, size=(P, 8)).astype(np.int64)
    rw = (rs.randint(0, 4, size=(P, 8)) * rs.randint(0, BIG // 3, size=(P, 8))).astype(np.int64)
    ri = (rs.randint(0, 3, size=(P, S, 5)) * rs.randint(0, BIG // 3, size=(P, S, 5))).astype(np.int64)
    genome = ''.join("ACGTN"[v] for v in rs.randint(0, 5, size=P))
    got = call_alone(rc, np.zeros((P, S, 5), dtype=np.int64), rw, ri, genome, S, 3, 60)
    want = call_arrays(rc.tolist(), rw.tolist(), ri.tolist(), genome, 0, S, 3, 60)
    for key in want:
        assert np.array_equal(got[key], want[key]), "P=%d random: %s" % (P, key)


def test_argument_checks():
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    ints = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(4)]
    byts = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(6)]
    p, u = ints[0].data_ptr(), byts[0].data_ptr()
    ok = lambda **kw: L.slk_pileup_call_qual_u8(*[kw.get(k, v) for k, v in (                                   # noqa: E731
        ('counts', ints[0].data_ptr()), ('ins', ints[1].data_ptr()), ('wcounts', ints[2].data_ptr()), ('wins', ints[3].data_ptr()),
        ('genome', byts[0].data_ptr()), ('G', 4), ('lo', 0), ('hi', 2), ('S', 1), ('md', 3), ('qmax', 60),
        ('letters', byts[1].data_ptr()), ('nlet', byts[2].data_ptr()), ('flags', byts[3].data_ptr()), ('letq', byts[4].data_ptr()),
        ('posq', byts[5].data_ptr()), ('stream', stream()))])
    assert ok() == _lib.SLK_OK and ok(qmax=1) == _lib.SLK_OK and ok(qmax=93) == _lib.SLK_OK
    for kw in (dict(qmax=0), dict(qmax=94), dict(wcounts=None), dict(wins=None), dict(letq=None), dict(posq=None), dict(S=17), dict(hi=5),
               dict(wcounts=ints[2].data_ptr() + 4)):
        assert ok(**kw) == _lib.SLK_ERR_INVALID_ARG, kw
    cnt = lambda **kw: L.slk_pileup_count_qual_u8(*[kw.get(k, v) for k, v in (                                 # noqa: E731
        ('q', u), ('ldq', 4), ('qlen', p), ('qual', u), ('roff', p), ('rows', p), ('fcodes', u), ('off', p), ('bytes', 8), ('status', p),
        ('minus', p), ('t0', p), ('G', 4), ('B', 1), ('lo', 0), ('hi', 2), ('S', 1), ('weights', u), ('counts', p), ('ins', p),
        ('wcounts', p), ('wins', p), ('stream', stream()))])
    for kw in (dict(qual=None), dict(weights=None), dict(wcounts=None), dict(wins=None), dict(S=0), dict(hi=5)):
        assert cnt(**kw) == _lib.SLK_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()


# ---- 4 - 6. the designed case through the public interface ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mapped():
    need_gpu()
    from sloika_amd import genome
    case = pileup_qual_cases.designed()
    idx = genome.Index([(pileup_qual_cases.CONTIG, case['genome'])], k=8, bin_width=512)  # every window is the whole contig
    res, strand, info, ops = idx.map(case['reads'], quals=case['quals'], ops=True)
    g = case['genome']
    pairs = []
    for b, read in enumerate(case['reads']):
        ws, we = int(info['window_start'][b]), int(info['window_end'][b])
        minus = strand[b] == '-'
        w = R.revcomp(g[ws:we]).decode('ascii') if minus else g[ws:we]
        row = [int(v) for v in ops.rows[b]]
        pairs.append((read, w, row, ops.codes(b), minus, we - row[4] if minus else ws + row[3], case['quals'][b]))
    G = len(g)
    tables = Q.pile(pairs, 0, G, 4, Q.weights_table())
    return {'case': case, 'idx': idx, 'map': (res, strand, info, ops), 'pairs': pairs, 'tables': tables}


def test_designed_case_through_the_public_interface(mapped):
    from sloika_amd import bio, genome
    case, idx, pairs = mapped['case'], mapped['idx'], mapped['pairs']
    res, strand, info, ops = mapped['map']
    G = len(case['genome'])
    name = pileup_qual_cases.CONTIG
    assert strand.tolist() == case['strands'] and (ops.status == 0).all()
    plain = idx.map(case['reads'], ops=True)                     # the qualities take no part in the mapping
    assert np.array_equal(plain[0], res) and plain[1].tolist() == strand.tolist() and plain[3].qual is None
    pile = genome.Pileup(idx, max_ins=4, weighted=True)
    assert pile.add(res, strand, info, ops).tolist() == [0] * len(pairs)
    counts, ins, wcounts, wins, views = mapped['tables']
    assert np.array_equal(pile.counts(), np.array(counts, dtype=np.int32))
    assert np.array_equal(pile.insertions(), np.array(ins, dtype=np.int32).reshape(G, 4, 5))
    assert np.array_equal(pile.weighted_counts(), np.array(wcounts, dtype=np.int32))
    assert np.array_equal(pile.weighted_insertions(), np.array(wins, dtype=np.int32).reshape(G, 4, 5))
    assert all(pile.columns(b).tolist() == views[b] for b in range(len(pairs)))
    cons = pile.consensus()
    want, parts, flags, quals, posq = Q.consensus(counts, wcounts, wins, case['genome'], 0, 3)
    assert cons.weighted and cons.sequences() == [(name, want.decode('ascii'))] == [(name, case['sample'])]
    assert cons.flags.tolist() == flags and cons.posq_dev.cpu().numpy().tolist() == posq
    flat = np.array([v for lq in quals for v in lq], dtype=np.uint8)
    got_q = cons.qualities()
    assert len(got_q) == 1 and got_q[0][0] == name and got_q[0][1].dtype == np.uint8 and np.array_equal(got_q[0][1], flat)
    assert len(flat) == len(case['sample'])
    assert cons.fastq() == bio.fastq_text([name], [case['sample']], [flat])
    assert bio.fastq_records(cons.fastq())[0][1] == case['sample']
    assert cons.variants(with_qual=True) == Q.variants(counts, wcounts, wins, case['genome'], 0, [0, G], [name])
    assert [v[:7] for v in cons.variants(with_qual=True)] == cons.variants()
    s = cons.summary()
    assert sorted(s) == ['covered', 'deleted', 'identity', 'inserted', 'substitutions'] and s['covered'] == sum(1 for f in flags if not f & R.LOW)
    # the majority call from the same tables follows the doubtful letters
    major = pile.consensus(weighted=False)
    mtext, _, mflags = R.consensus(counts, ins, case['genome'], 0, 3)
    assert not major.weighted and major.sequences() == [(name, mtext.decode('ascii'))] and major.flags.tolist() == mflags
    assert major.sequences()[0][1] != case['sample']
    assert major.variants() == R.variants(counts, ins, case['genome'], 0, [0, G], [name])
    # min_qual and the one-call form
    cut, cut_cons = genome.pileup(idx, res, strand, info, ops, weighted=True, min_qual=10, qmax=40)
    c2 = Q.pile(pairs, 0, G, 4, Q.weights_table(10, 40))
    assert np.array_equal(cut.weighted_counts(), np.array(c2[2], dtype=np.int32))
    assert np.array_equal(cut.weighted_insertions(), np.array(c2[3], dtype=np.int32).reshape(G, 4, 5))
    w2 = Q.consensus(c2[0], c2[2], c2[3], case['genome'], 0, 3, 40)
    assert cut_cons.sequences() == [(name, w2[0].decode('ascii'))]
    assert np.array_equal(cut_cons.qualities()[0][1], np.array([v for lq in w2[3] for v in lq], dtype=np.uint8))
    # an unweighted Pileup ignores ops.qual: today's tables
    old = genome.Pileup(idx, max_ins=4)
    old.add(res, strand, info, ops)
    assert np.array_equal(old.counts(), pile.counts()) and np.array_equal(old.insertions(), pile.insertions())


def test_batching_does_not_show(mapped):
    from sloika_amd import genome
    case, idx = mapped['case'], mapped['idx']
    res, strand, info, ops = mapped['map']
    G, B = len(case['genome']), len(case['reads'])
    name = pileup_qual_cases.CONTIG
    whole = genome.Pileup(idx, max_ins=3, weighted=True)
    whole.add(res, strand, info, ops)
    tables = lambda p: (p.counts(), p.insertions(), p.weighted_counts(), p.weighted_insertions())          # noqa: E731
    W = tables(whole)
    same = lambda p, sl=slice(None): all(np.array_equal(a, b[sl]) for a, b in zip(tables(p), W))          # noqa: E731
    halves = genome.Pileup(idx, max_ins=3, weighted=True)
    for lo, hi in ((0, B // 2), (B // 2, B)):
        part = idx.map(case['reads'][lo:hi], quals=case['quals'][lo:hi], ops=True)
        assert halves.add(*part).tolist() == [0] * (hi - lo)
    assert same(halves)
    masks = genome.Pileup(idx, max_ins=3, weighted=True)
    first = np.arange(B) < B // 2
    assert masks.add(res, strand, info, ops, keep=first).tolist() == [0 if k else 1 for k in first]
    masks.add(res, strand, info, ops, keep=~first, qual=ops.qual)
    assert same(masks)
    for region in ((name, 0, 100), (0, 95, 333), (name, 300, G), (0, 17, 17)):
        part = genome.Pileup(idx, region=region, max_ins=3, weighted=True)
        part.add(res, strand, info, ops)
        assert same(part, slice(region[1], region[2])), region
        cons = part.consensus()
        if region[2] == region[1]:
            assert cons.sequences() == [] and cons.qualities() == [] and cons.fastq() == ""
            continue
        want = Q.consensus(W[0][region[1]:region[2]], W[2][region[1]:region[2]], W[3][region[1]:region[2]], case['genome'],
                           region[1], 3)
        assert cons.sequences() == [(name, want[0].decode('ascii'))]
        assert np.array_equal(cons.qualities()[0][1], np.array([v for lq in want[3] for v in lq], dtype=np.uint8))


def test_refused_pairs_add_nothing_to_any_table():
    rs = np.random.RandomState(9)
    G = 260
    genome = ''.join("ACGT"[v] for v in rs.randint(0, 4, size=G))
    rnd = lambda n: [int(v) for v in rs.choice([M, X, I, D], size=n, p=[0.7, 0.1, 0.1, 0.1])]     # noqa: E731
    pairs = with_quals(rs, [T.fwd_pair(rs, rnd(80), k % 2 == 1, 10 + 20 * k) for k in range(6)])
    want_status = [0] * 6
    q, r, row, codes, minus, t0, qual = pairs[1]
    row = list(row)
    row[5], row[7] = row[5] + 1, row[7] - 1
    if row[7] < 0:
        row[5], row[7] = row[5] - 2, row[7] + 2
    pairs[1], want_status[1] = (q, r, row, codes, minus, t0, qual), R.BAD_SUM
    q, r, row, codes, minus, t0, qual = pairs[3]
    pairs[3], want_status[3] = (q, r, row, codes, minus, G - (row[4] - row[3]) + 1, qual), R.POSITION
    q, r, row, codes, minus, t0, qual = pairs[4]
    pairs[4], want_status[4] = (q, r, row, codes, minus, -1, qual), R.POSITION
    weights = Q.weights_table()
    got = launch(pairs, G, genome, 0, G, 4, weights, min_depth=1)
    assert got['status'].tolist() == want_status
    assert [R.check_pair(p[2], p[3], len(p[0]), len(p[1]), p[5], G) for p in pairs] == want_status
    live = [p for p, s in zip(pairs, want_status) if s == 0]
    compare(got, model(live, genome, 0, G, 4, weights, True, 1), "refusals")


def test_refusals_by_name(mapped):
    from sloika_amd import genome
    case, idx = mapped['case'], mapped['idx']
    res, strand, info, ops = mapped['map']
    plain = idx.map(case['reads'][:6], ops=True)
    weighted = genome.Pileup(idx, weighted=True)
    with pytest.raises(ValueError, match="weighted pileup needs the reads' qualities"):
        weighted.add(*plain)
    assert not weighted.counts().any() and not weighted.weighted_counts().any()
    with pytest.raises(ValueError, match="qual= must be a contiguous uint8 device tensor"):
        weighted.add(*plain, qual=ops.qual)                      # the qualities of another batch: the wrong shape
    unweighted = genome.Pileup(idx)
    unweighted.add(res, strand, info, ops)
    with pytest.raises(ValueError, match=r"consensus\(weighted=True\) needs a Pileup made with weighted=True"):
        unweighted.consensus(weighted=True)
    with pytest.raises(ValueError, match=r"weighted_counts\(\) needs"):
        unweighted.weighted_counts()
    with pytest.raises(ValueError, match=r"qualities\(\) needs a weighted call"):
        unweighted.consensus().qualities()
    with pytest.raises(ValueError, match=r"with_qual=True\) needs a weighted call"):
        unweighted.consensus().variants(with_qual=True)
    short = [q.copy() for q in case['quals'][:6]]
    short[4] = short[4][:-1]
    with pytest.raises(ValueError, match="quals= of read r4 has %d values for %d letters" % (len(short[4]), len(case['reads'][4]))):
        idx.map(case['reads'][:6], quals=short, names=["r%d" % k for k in range(6)])
    with pytest.raises(ValueError, match="quals= holds 5 arrays for 6 queries"):
        idx.map(case['reads'][:6], quals=short[:5])
    # the memory check counts both pairs of tables
    G = len(case['genome'])
    one = G * (8 + 5 * 4) * 4
    genome.Pileup(idx, max_ins=4, memory_limit=one)
    genome.Pileup(idx, max_ins=4, memory_limit=2 * one, weighted=True)
    with pytest.raises(ValueError, match="two pairs of tables .* region="):
        genome.Pileup(idx, max_ins=4, memory_limit=2 * one - 1, weighted=True)
    with pytest.raises(ValueError, match="qmax"):
        genome.Pileup(idx, weighted=True, qmax=94)
    with pytest.raises(ValueError, match="weights="):
        genome.Pileup(idx, weighted=True, weights=np.zeros(255, dtype=np.uint8))


# ---- 7. map_paths(conf=) -------------------------------------------------------------------------------------------------------------------

def test_map_paths_with_conf_keeps_the_rows_and_leaves_the_qualities_on_the_device():
    torch = need_gpu()
    from sloika_amd import bio, genome
    klen, rs = 5, np.random.RandomState(8)
    nst = 4 ** klen
    lens = [0, 1, 40, 300, 120, 77]
    paths = np.zeros((len(lens), max(lens) + 2), dtype=np.int32)
    for b, n in enumerate(lens):
        s = rs.randint(0, nst)
        for t in range(n):
            s = (s * 4) % nst + rs.randint(0, 4) if rs.uniform() < 0.9 else rs.randint(0, nst)
            paths[b, t] = s
    pd, ld = dev(paths), dev(np.asarray(lens, dtype=np.int32))
    conf = dev(rs.uniform(1e-6, 1.0 - 1e-6, size=paths.shape).astype(np.float64))
    called = bio.paths_to_bases_qual(pd, ld, conf, klen, "ACGT", qmax=50)
    contigs = []
    for b, (c, _) in enumerate(called):
        m = align_cases.mutate(rs, c)
        contigs.append(("g%d" % b, align_cases.random_seq(rs, 100 + 37 * b) + (align_cases.revcomp(m) if b % 2 else m)
                        + align_cases.random_seq(rs, 150)))
    idx = genome.Index(contigs, k=10, bin_width=64)
    want = idx.map_paths(pd, ld, klen, ops=True)
    got = idx.map_paths(pd, ld, klen, ops=True, conf=conf, qmax=50)
    assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist() and got[3].tolist() == want[3].tolist()
    assert all(np.array_equal(got[2][key], want[2][key]) for key in want[2])
    assert (got[0][3:, 0] > 0).all()                             # the longer calls are placed
    ops = got[4]
    assert want[4].qual is None and ops.qual.dtype == torch.uint8 and tuple(ops.qual.shape) == (len(lens), ops.ldq)
    assert ops.qual.is_cuda
    host = ops.qual.cpu().numpy()
    for b, (text, q) in enumerate(called):
        assert np.array_equal(host[b, :len(text)], q), b
        assert ops.queries()[b] == text.encode('ascii')
    assert max(int(q.max()) for _, q in called if len(q)) <= 50 and len({int(v) for _, q in called for v in q}) > 5
    # and a weighted pileup takes them as they lie
    pile = genome.Pileup(idx, weighted=True, qmax=50)
    status = pile.add(got[0], got[1], got[2], ops)
    assert (status[3:] == 0).all()
    wc, cn = pile.weighted_counts().astype(np.int64), pile.counts().astype(np.int64)
    assert cn[:, :6].sum() > 0 and 0 < wc[:, :6].sum() <= 50 * cn[:, :6].sum()
