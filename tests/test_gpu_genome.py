"""Locating calls on a genome on the device: csrc/genome_map.hip through sloika_amd.genome against the dict model of
tests/genome_ref.py (keys and votes: EQUAL, integer for integer) and against the exact aligner over the whole contig
(align.align_batch, itself pinned to tests/align_ref.py) for the placement.  Shapes are the smallest at which each kernel can go
wrong: contigs of 700, 20000 and 3000 letters, k = 10 and W = 64 unless a test says otherwise."""
import os

import numpy as np
import pytest

from tests import align_cases, align_ref, genome_ref
from tests.gpu_util import need_gpu, dev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, W = 10, 64


def three_contigs(seed=40):
    rs = np.random.RandomState(seed)
    return [("c700", align_cases.random_seq(rs, 700)), ("c20000", align_cases.random_seq(rs, 20000)),
            ("c3000", align_cases.random_seq(rs, 3000))]


@pytest.fixture(scope="module")
def placed():
    """The three contigs, their index and the model's table, shared and left unchanged."""
    need_gpu()
    from sloika_amd import genome
    contigs = three_contigs()
    return contigs, genome.Index(contigs, k=K, bin_width=W), genome_ref.occurrences(contigs, K)


# ---- 1. keys -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 10, 15])
def test_keys_equal_the_model(k, tmp_path):
    need_gpu()
    from sloika_amd import genome
    rs = np.random.RandomState(41)
    contigs = three_contigs() + [("short", align_cases.random_seq(rs, k - 1)),
                                 ("enn", "N" + align_cases.random_seq(rs, 200) + "N" * 20 + align_cases.random_seq(rs, 200) + "N"),
                                 ("last", align_cases.random_seq(rs, 2 * k))]
    want, nvalid = genome_ref.genome_keys(contigs, k)
    idx = genome.Index(contigs, k=k)
    assert idx.nvalid == nvalid and idx.G == len(want)
    got = idx.keys.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, np.sort(want))          # the keys hold their position: equal sorted = equal
    # every contig's last k - 1 positions are invalid, and so is all of the contig shorter than k
    code = want >> 32
    for c in range(len(contigs)):
        assert (code[max(idx.offsets[c], idx.offsets[c + 1] - (k - 1)):idx.offsets[c + 1]] == genome_ref.INVALID).all()
    assert (np.sort(got)[nvalid:] >> 32 == genome_ref.INVALID).all() and (got[:nvalid] >> 32 < genome_ref.INVALID).all()
    if k == 10:                                                   # the same genome from a FASTA file in lower case, as a dict, as bytes
        path = tmp_path / "g.fa"
        path.write_text(genome.fasta([(n, s.lower()) for n, s in contigs]))
        again = genome.Index.from_fasta(str(path), k=k)
        assert again.names == [n for n, _ in contigs] and np.array_equal(again.keys.cpu().numpy(), got) and again.nvalid == nvalid
        as_dict = genome.Index({n: s.encode() for n, s in contigs}, k=k)
        assert np.array_equal(as_dict.keys.cpu().numpy(), got)


# ---- 2. the seed stage ------------------------------------------------------------------------------------------------------------

def seed_genome():
    """The three contigs, a contig with a 12-fold tandem repeat whose copies are broken so that one k-mer occurs exactly 8 and another
    9 times, and a contig that holds one stretch twice and another on both strands."""
    rs = np.random.RandomState(42)
    contigs = three_contigs()
    unit = align_cases.random_seq(rs, 40)
    copies = []
    for c in range(12):
        u = list(unit)
        if c in (1, 4, 7, 10):                                    # breaks unit[0:10] in four copies: 8 occurrences left
            u[5] = 'ACGT'[('ACGT'.index(u[5]) + 1) % 4]
        if c in (2, 5, 8):                                        # breaks unit[20:30] in three copies: 9 left
            u[25] = 'ACGT'[('ACGT'.index(u[25]) + 1) % 4]
        copies.append(''.join(u))
    contigs.append(("tandem", align_cases.random_seq(rs, 150) + ''.join(copies) + align_cases.random_seq(rs, 150)))
    twice, both = align_cases.random_seq(rs, 60), align_cases.random_seq(rs, 60)
    r = lambda n: align_cases.random_seq(rs, n)
    contigs.append(("dup", r(300) + twice + r(500) + twice + r(300) + both + r(400) + align_cases.revcomp(both) + r(200)))
    return contigs, unit, twice, both


def seed_queries(contigs, unit, twice, both):
    rs = np.random.RandomState(43)
    c0, c1, c2 = contigs[0][1], contigs[1][1], contigs[2][1]
    qs = []
    for n in (0, 1, K - 1, K, K + 1, 30, 63, 64, 65):             # exact copies of a locus of c20000
        qs.append(c1[5000:5000 + n])
    qs.append(align_cases.mutate(rs, c1[7000:7300])[:300])
    qs.append(align_cases.revcomp(align_cases.mutate(rs, c1[9000:11100])[:2000]))
    qs.append(c1[12000:12040] + "N" + c1[12041:12080] + "NN" + c1[12082:12130])       # Ns break the k-mers over them
    qs.append("N" * 25)
    qs.append(align_cases.random_seq(rs, 80) + c0[:120])                              # overhangs the genome's start: p - i < 0
    qs.append(contigs[-1][1][-120:] + align_cases.random_seq(rs, 80))                 # ... and its end
    qs.append(align_cases.random_seq(rs, 50) + c2[:100])                              # overhangs a contig's start
    qs.append(c0[-60:] + c1[:60])                                                     # a locus that straddles two contigs
    qs.append(contigs[3][1][140:340])                                                 # into the tandem repeat: max_occ decides
    qs.append(unit + unit)
    qs.append(twice)                                                                  # two loci, equal votes: the smaller bin
    qs.append(both)                                                                   # equal votes on both strands
    qs.append(align_cases.random_seq(rs, 200))                                        # unrelated
    return qs


def test_seed_stage_equals_the_model():
    need_gpu()
    from sloika_amd import genome
    contigs, unit, twice, both = seed_genome()
    table = genome_ref.occurrences(contigs, K)
    assert len(table[genome_ref.kmer_code(unit[:10])]) == 8 and len(table[genome_ref.kmer_code(unit[20:30])]) == 9
    idx = genome.Index(contigs, k=K, bin_width=W, max_occ=8)
    qs = seed_queries(contigs, unit, twice, both)
    want = np.array([genome_ref.seed(table, q, K, W, 8) for q in qs], dtype=np.int32)
    got = idx.seed(qs)
    assert got.dtype == np.int32 and got.shape == (len(qs), 2, 4)
    bad = [(b, len(qs[b]), got[b].tolist(), want[b].tolist()) for b in range(len(qs)) if not np.array_equal(got[b], want[b])]
    assert not bad, bad[:5]
    # the batch holds what it claims
    named = dict(zip(("tandem", "units", "twice", "both", "random"), range(len(qs) - 5, len(qs))))
    assert (want[:3, :, 1] == 0).all() and want[2, 0, 3] == 0 and want[3, 0, 1] >= 1          # shorter than k: no vote; k letters: one seed
    assert want[named["tandem"], 0, 3] < 200 - K + 1                                   # some k-mers were skipped for max_occ
    t = want[named["twice"], 0]
    assert t[1] == t[2] >= 51                                                          # the second locus has as many votes
    assert want[named["both"], 0, 1] == want[named["both"], 1, 1] >= 51
    assert want[10, 1, 1] > 50 > want[10, 0, 1]                                        # the reverse-complemented read votes on '-'
    # the same queries in reversed order and alone give the same rows
    assert np.array_equal(idx.seed(qs[::-1])[::-1], got)
    for b in (0, 9, 10, named["twice"]):
        assert np.array_equal(idx.seed([qs[b]])[0], got[b]), b
    # both loci of `both` tie across the strands: '+' is chosen
    res, strand, info = idx.map([both])
    assert strand[0] == '+' and info['contig'][0] == 4 and res[0, 0] == 60


# ---- 3. placement ------------------------------------------------------------------------------------------------------------------

def placement_candidates(contigs):
    """(query, contig index, planted strand): 12 % error copies of loci, 100..2000 letters, both strands, some flush with a contig end."""
    rs = np.random.RandomState(44)
    lengths = [100, 110, 120, 135, 150, 170, 200, 240, 300, 380, 450, 520, 600, 700, 800, 900, 1000, 1150, 1300, 1450, 1600, 1750, 1900,
               2000]
    out = []
    for j, n in enumerate(lengths):
        c = (0, 1, 2, 1)[j % 4] if n <= 650 else (1, 2, 1)[j % 3]
        seq = contigs[c][1]
        at = 0 if j % 6 == 1 else len(seq) - n if j % 6 == 4 else rs.randint(0, len(seq) - n + 1)
        q = align_cases.mutate(rs, seq[at:at + n])
        minus = j % 2 == 1
        out.append((align_cases.revcomp(q) if minus else q, c, '-' if minus else '+'))
    return out


@pytest.fixture(scope="module")
def admitted(placed):
    """The candidates the MODEL places clearly (votes >= 4, second <= votes / 2), decided on the CPU before any launch."""
    contigs, idx, table = placed
    cands = placement_candidates(contigs)
    keep = []
    for q, c, s in cands:
        choice = genome_ref.choose_strand(genome_ref.seed(table, q, K, W, 64), 3)
        if choice is not None and choice[1][1] >= 4 and 2 * choice[1][2] <= choice[1][1]:
            keep.append((q, c, s, choice[1]))
    assert len(keep) >= 0.9 * len(cands), "the generator admits too few of its candidates: the test would be vacuous"
    return keep


def test_placement_equals_the_exact_aligner_over_the_contig(placed, admitted):
    from sloika_amd import align
    contigs, idx, _ = placed
    qs = [a[0] for a in admitted]
    res, strand, info = idx.map(qs)
    want, wstrand = align.align_batch(qs, [contigs[a[1]][1] for a in admitted], both_strands=True)
    assert strand.tolist() == wstrand.tolist() == [a[2] for a in admitted]
    assert info['contig'].tolist() == [a[1] for a in admitted]
    bad = [(b, res[b].tolist(), want[b].tolist()) for b in range(len(qs)) if not np.array_equal(res[b], want[b])]
    assert not bad, bad[:5]
    assert (info['edge'] == 0).all() and info['votes'].tolist() == [a[3][1] for a in admitted]
    assert res[:, 3].min() <= 3 and any(res[b, 4] >= len(contigs[a[1]][1]) - 3 for b, a in enumerate(admitted))      # flush with both ends
    # a handful of the shortest, planted in the 700-letter contig, against the traceback oracle itself
    short = [b for b, a in enumerate(admitted) if a[1] == 0][:3]
    assert len(short) >= 2
    for b in short:
        q, c, s, _ = admitted[b]
        ref = contigs[c][1]
        if s == '+':
            w = align_ref.align(q, ref)
        else:
            w = align_ref.align(q, align_cases.revcomp(ref))
            w[3], w[4] = len(ref) - w[4], len(ref) - w[3]
        assert res[b].tolist() == w, b


# ---- 4. unmapped and refusals ---------------------------------------------------------------------------------------------------------

def test_unmapped_min_votes_and_refusals(placed, admitted):
    torch = need_gpu()
    from sloika_amd import _lib, genome
    contigs, idx, table = placed
    rs = np.random.RandomState(45)
    unrelated = [align_cases.random_seq(rs, n) for n in (200, 150, 90)]
    for q in unrelated:                                           # the model: neither strand reaches three votes
        assert max(row[1] for row in genome_ref.seed(table, q, K, W, 64)) < 3
    res, strand, info = idx.map(unrelated + [admitted[0][0]])
    assert info['contig'].tolist() == [-1, -1, -1, admitted[0][1]] and not res[:3].any() and res[3, 0] > 0
    assert strand[:3].tolist() == ['+'] * 3
    # min_votes at votes = min_votes and votes = min_votes - 1
    q, c, s, row = admitted[0]
    res, _, info = idx.map([q], min_votes=row[1])
    assert info['contig'][0] == c and res[0, 0] > 0 and info['votes'][0] == row[1]
    res, _, info = idx.map([q], min_votes=row[1] + 1)
    assert info['contig'][0] == -1 and not res.any() and info['votes'][0] == row[1]
    # a device-side length beyond its launch bound: bin = -1 from the entry, ValueError from Python
    qd = dev(np.frombuffer(q.encode(), dtype=np.uint8).reshape(1, -1).copy())
    qlen = dev(np.array([len(q)], dtype=np.int32))
    with pytest.raises(ValueError, match="longer than the bound"):
        idx._seed_device(qd, len(q), qlen, len(q) - 1)
    L = _lib.lib()
    out = torch.zeros((1, 2, 4), dtype=torch.int32, device=qd.device)
    nbytes = L.slk_genome_seed_workspace_bytes(1, len(q) - 1, idx.G, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qd.device)
    assert L.slk_genome_seed_votes_u8(qd.data_ptr(), len(q), qlen.data_ptr(), 1, len(q) - 1, idx.keys.data_ptr(), idx.nvalid, idx.G, K, W,
                                      64, out.data_ptr(), ws.data_ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[0].tolist() == [[-1, 0, 0, 0], [-1, 0, 0, 0]]
    assert L.slk_genome_seed_votes_u8(qd.data_ptr(), len(q), qlen.data_ptr(), 1, len(q), idx.keys.data_ptr(), idx.nvalid, idx.G, K, 48,
                                      64, out.data_ptr(), ws.data_ptr(), nbytes, None) == _lib.SLK_ERR_INVALID_ARG
    assert L.slk_genome_seed_votes_u8(qd.data_ptr(), len(q), qlen.data_ptr(), 1, len(q), idx.keys.data_ptr(), idx.nvalid, idx.G, K, W,
                                      64, out.data_ptr(), ws.data_ptr(), 16, None) == _lib.SLK_ERR_WORKSPACE
    with pytest.raises(ValueError, match="may not exceed"):
        idx.seed(["A" * (65536 - W + 1)])
    # a window of more than 65535 letters is refused by name
    big = align_cases.random_seq(rs, 70000)
    bidx = genome.Index([("big", big)], k=K, bin_width=W)
    read = big[30000:31000]
    res, _, info = bidx.map([read], names=["read7"])
    assert res[0].tolist() == [1000, 0, 1000, 30000, 31000, 1000, 0, 0, 0] and info['edge'][0] == 0
    with pytest.raises(ValueError, match="read7 is [0-9]+ letters"):
        bidx.map([read], drift=40.0, names=["read7"])


# ---- 5. edge ---------------------------------------------------------------------------------------------------------------------------

def test_edge_flags_an_alignment_that_leaves_its_window():
    """A read with a 200-letter deletion: 1000 letters at contig position 1024 (a multiple of W), then the 600 letters that follow 200
    further on.  The first part has more seeds, its diagonal 1024 + 65536 is a bin's first, so the bins of it tie and the smaller
    is taken: without drift the window ends at 1024 + W + 1600 + W = 2752, 72 letters short of the read's end at 2824 -- the
    alignment crosses the gap (528 matches behind it are worth more than the gap's 202), runs into the window's end and leaves
    letters unaligned.  The default drift adds ceil(1600 / 16) = 100: the window reaches 2852 and holds all of it."""
    need_gpu()
    from sloika_amd import align, genome
    contig = align_cases.random_seq(np.random.RandomState(46), 4000)
    read = contig[1024:2024] + contig[2224:2824]
    idx = genome.Index([("c", contig)], k=K, bin_width=W)
    res, strand, info = idx.map([read], drift=0.0)
    assert info['window_end'][0] == 2752 and info['edge'][0] == 1 and strand[0] == '+'
    assert res[0, 3] == 1024 and res[0, 4] == 2752 and res[0, 2] == 1600 - 72 and res[0, 8] == 200
    res, strand, info = idx.map([read])
    want, wstrand = align.align_batch([read], [contig], both_strands=True)
    assert info['window_end'][0] == 2852 and info['edge'][0] == 0 and np.array_equal(res, want) and strand[0] == wstrand[0] == '+'
    assert res[0].tolist() == [1600 - 202, 0, 1600, 1024, 2824, 1600, 0, 0, 200]
    # the same on the other strand: the window's START is the end that is left
    res, strand, info = idx.map([align_cases.revcomp(read)], drift=0.0)
    assert info['edge'][0] == 1 and strand[0] == '-' and res[0, 3] == 1024 and res[0, 4] == 2752 and res[0, 1] == 72


# ---- 6. split launches -----------------------------------------------------------------------------------------------------------------

def test_split_launches_give_the_rows_of_one(placed, admitted):
    from sloika_amd import align, genome
    contigs, idx, _ = placed
    qs = [a[0] for a in admitted]
    res, strand, info = idx.map(qs)
    lens = [len(q) for q in qs]
    wlens = info['window_end'] - info['window_start']
    assert wlens.max() > align.PASS_WIDTH
    limit = next((v for v in range(24 * max(lens), 24 * max(lens) * len(qs), 24 * max(lens) // 16)
                  if len(genome.align_runs(lens, wlens, v)) == 3), None)
    assert limit is not None
    res3, strand3, info3 = idx.map(qs, workspace_limit=limit)
    assert np.array_equal(res3, res) and strand3.tolist() == strand.tolist()
    assert all(np.array_equal(info3[key], info[key]) for key in info)
    # ... and so does another order of the batch
    order = np.random.RandomState(47).permutation(len(qs))
    res_p, strand_p, _ = idx.map([qs[j] for j in order], workspace_limit=limit)
    assert np.array_equal(res_p, res[order]) and strand_p.tolist() == strand[order].tolist()


# ---- 7. paths ------------------------------------------------------------------------------------------------------------------------------

def test_map_paths_equals_map_on_the_called_strings():
    need_gpu()
    from sloika_amd import align, bio, genome
    P = align.PASS_WIDTH
    klen, rs = 5, np.random.RandomState(8)
    nst = 4 ** klen
    lens = [0, 1, 40, 300, P + 30, 120, 77]
    paths = np.zeros((len(lens), max(lens) + 2), dtype=np.int32)
    for b, n in enumerate(lens):
        s = rs.randint(0, nst)
        for t in range(n):
            s = (s * 4) % nst + rs.randint(0, 4) if rs.uniform() < 0.9 else rs.randint(0, nst)
            paths[b, t] = s
    pd, ld = dev(paths), dev(np.asarray(lens, dtype=np.int32))
    called = bio.paths_to_bases(pd, ld, klen, "ACGT", always_move=True)
    # a genome that holds an error copy of every call, every other one on the other strand
    contigs = []
    for b, c in enumerate(called):
        m = align_cases.mutate(rs, c)
        contigs.append(("g%d" % b, align_cases.random_seq(rs, 100 + 37 * b) + (align_cases.revcomp(m) if b % 2 else m)
                        + align_cases.random_seq(rs, 150)))
    idx = genome.Index(contigs, k=K, bin_width=W)
    res, strand, info, nbases = idx.map_paths(pd, ld, klen)
    want, wstrand, winfo = idx.map(called)
    assert nbases.tolist() == [len(c) for c in called]
    assert np.array_equal(res, want) and strand.tolist() == wstrand.tolist()
    assert all(np.array_equal(info[key], winfo[key]) for key in info)
    assert info['contig'].tolist()[3:] == [3, 4, 5, 6] and strand.tolist()[3:] == ['-', '+', '-', '+'] and info['contig'][0] == -1
    rows = genome.samacc_rows(idx, res, strand, info, nbases, names=["r%d" % b for b in range(len(lens))])
    assert len(rows) >= 4 and list(rows[0])[:2] == ['reference', 'query'] and all(r['reference'] == "g" + r['query'][1:] for r in rows)
    assert align.summary(rows)['mapped'] == len(rows) and all(0.7 < r['accuracy'] <= 1.0 for r in rows)


# ---- 8, 9. real reads ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def real():
    """This build's calls of the two example reads and a genome that holds ONT's stored basecalls of them: called_3 as it is and
    the reverse complement of called_5, each between seeded flanks."""
    need_gpu()
    from sloika_amd import basecall, bio, genome, models
    g = np.load(os.path.join(GOLDEN, "reads.npz"))
    calc_post = models.from_weights_npz(os.path.join(GOLDEN, "pretrained_weights.npz")).compile()
    kmers = bio.all_kmers(5)
    calls, signals = [], []
    for n in (3, 5):
        dig, off, rng, _rate = g["meta_%d" % n]
        signal = (g["adc_%d" % n].astype(np.float64) + off) * (rng / dig)
        _, _, call, _ = basecall.raw_read_worker(calc_post, signal, trim=(200, 10), kmer_len=5, skip=5.0, name="read%d" % n)
        calls.append(bio.kmers_to_sequence([kmers[i] for i in call], always_move=True))
        signals.append(signal)
    rs = np.random.RandomState(48)
    stored = [g["called_3"].tobytes().decode(), align_cases.revcomp(g["called_5"].tobytes().decode())]
    flanks = [(1500, 900), (700, 2100)]
    contigs = [("chrA", align_cases.random_seq(rs, flanks[0][0]) + stored[0] + align_cases.random_seq(rs, flanks[0][1])),
               ("chrB", align_cases.random_seq(rs, flanks[1][0]) + stored[1] + align_cases.random_seq(rs, flanks[1][1]))]
    return calls, signals, contigs, stored, flanks, genome.Index(contigs), calc_post


def test_real_reads_land_where_their_stored_calls_lie(real):
    from sloika_amd import align, genome
    calls, signals, contigs, stored, flanks, idx, _ = real
    assert (idx.k, idx.bin_width) == (14, 256)
    names = ["read3.fast5", "read5"]
    res, strand, info = idx.map(calls, names=names)
    assert strand.tolist() == ['+', '-'] and info['contig'].tolist() == [0, 1] and (info['edge'] == 0).all()
    want, wstrand = align.align_batch(calls, [c[1] for c in contigs], both_strands=True)
    assert np.array_equal(res, want) and wstrand.tolist() == ['+', '-']
    for b in range(2):                                            # on the planted stretch, and most of it
        lo, hi = flanks[b][0], flanks[b][0] + len(stored[b])
        assert lo - 20 <= res[b, 3] < lo + 0.1 * len(stored[b]) and hi - 0.1 * len(stored[b]) < res[b, 4] <= hi + 20
    assert (info['votes'] > 20 * np.maximum(info['second'], 1)).all()
    # the references of get_refs: a host slice of the genome under the same arithmetic, holding the aligned span
    records, strand_list = genome.read_references(idx, res, strand, info, [len(c) for c in calls], names, pad=50)
    assert [n for n, _ in records] == ["read3", "read5"] and strand_list == ["read3.fast5.fast5", "read5.fast5"]
    for b, (_, seq) in enumerate(records):
        qs, qe, r0, r1 = (int(v) for v in res[b, 1:5])
        assert seq == genome_ref.read_reference(contigs[b][1], qs, qe, r0, r1, strand[b], len(calls[b]), 50)
        span = contigs[b][1][r0:r1]
        assert (span if strand[b] == '+' else align_cases.revcomp(span)) in seq
        assert len(seq) >= r1 - r0 + 100
    assert genome.fasta(records).count(">") == 2
    rows = genome.samacc_rows(idx, res, strand, info, [len(c) for c in calls], names=names)
    assert [r['reference'] for r in rows] == ["chrA", "chrB"] and all(0.8 < r['accuracy'] < 1.0 for r in rows)
    # the drift of the diagonal along each alignment, from 400-letter pieces of the call placed on their own: the only real-data
    # evidence for the default drift of 1 / 16 (design/genome_map.md, Measured)
    for b in range(2):
        call = calls[b] if strand[b] == '+' else align_cases.revcomp(calls[b])
        pieces = [call[j:j + 400] for j in range(0, len(call) - 399, 400)]
        pres, pstrand, pinfo = idx.map(pieces)
        ok = (pinfo['contig'] == b) & (pstrand == '+')
        diag = (pres[:, 3] - pres[:, 1] - 400 * np.arange(len(pieces)))[ok]
        net = int(res[b, 8]) - int(res[b, 7])
        print("read %d: %d letters, strand %s, deletions - insertions = %d, diagonal of %d / %d pieces spans %d (%.4f of the length)"
              % ((3, 5)[b], len(call), strand[b], net, int(ok.sum()), len(pieces), int(diag.max() - diag.min()),
                 float(diag.max() - diag.min()) / len(call)))
        assert ok.sum() >= 0.8 * len(pieces)
        assert diag.max() - diag.min() <= idx.bin_width + len(call) / 16.0          # inside the slack the default drift gives


def test_references_feed_the_raw_remap(real):
    """The hand-over alone: the (name, sequence) records of read_references are what chunkify_raw.raw_remap_many takes as `refs`."""
    from sloika_amd import chunkify_raw, genome, util
    calls, signals, contigs, stored, flanks, idx, calc_post = real
    res, strand, info = idx.map(calls[1:])
    records, _ = genome.read_references(idx, res, strand, info, [len(calls[1])], ["read5"])
    assert len(records) == 1
    signal = util.trim_array(signals[1].astype(np.float32), 200, 10)
    (score, table, path, seq), = chunkify_raw.raw_remap_many([records[0][1]], [signal], 1e-5, 5, (25.0, 25.0), 5.0, calc_post=calc_post)
    assert np.isfinite(score) and len(seq) == len(records[0][1]) - 4 and len(path) == -(-len(signal) // 5)
    assert path[-1] - path[0] > 0.8 * len(calls[1])              # the mapping walks through the read's part of the reference
