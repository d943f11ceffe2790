"""The lattice marginals on the device (csrc/lattice_marginals.hip, slk_paths_to_bases_qual, the *_qual entries of
pipeline.Basecaller; design/lattice_marginals.md), through the C ABI.

Integer outputs and the float32 score are compared bit for bit: with slk_viterbi_kmer_f32 on the same input, and with the numpy
Viterbi of tests/lattice_ref.py on the device's own slk_log_post_f32 output.  The float64 outputs are compared with the same oracle
in np.longdouble on slk_prepare_post_f32's values.  The yardstick is E_m, the float64 oracle's largest distance from that truth over
the cases below (gamma, conf, and log Z per row), computed here on the CPU; the device may lie 4 E_m away (the allowance
design/forward_score.md 5 gives a float64 device recursion), gamma another 2^-24 gamma for its one rounding to float32.
Measured on an MI355X (one run): E_m 2.489e-15; the largest device distance 1.05 E_m (conf), 0.19 E_m (log Z / T), gamma within its
rounding to float32 (design/lattice_marginals.md 5)."""
import numpy as np
import pytest

from tests import lattice_ref as lr
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu

LD = np.longdouble
ALLOW = 4.0
SENT_F, SENT_I, SENT_D = np.float32(-7.25), np.int32(-77), np.float64(-7.25)


def make_post(seed, T, B, S, sharp):
    rs = np.random.RandomState(seed)
    p = rs.dirichlet(np.ones(S) * (0.05 if sharp else 1.0), size=T * B).astype(np.float32)
    return np.ascontiguousarray(p.reshape(T, B, S))


def zero_post():
    """nbase 4, klen 3, min_prob 0: row 3 is exactly 0 but for state AAA, which the rows around it cannot reach; the best path has to
    cross row 3 in a state that weighs exactly 0 (every other crossing pays the floor of the log twice)."""
    T, S = 8, 65
    q, w = 6, 3 * 16 + 0 * 4 + 1                            # ACG ... TAC: two letters on, by a step and a skip through row 3
    p = np.full((T, 1, S), 1e-20, dtype=np.float32)
    for i, col in enumerate([1 + q, 0, 0, None, 1 + w, 0, 0, 0]):
        if col is not None:
            p[i, 0, col] = 1.0
    p[3] = 0.0
    p[3, 0, 1 + 0] = 1.0
    return p


# name -> (nbase, klen, T, B, skip_pen, min_prob, lens, sharp)
CASES = {
    "n64_t1": (4, 3, 1, 1, 0.0, 1e-5, None, False),
    "n64_t2": (4, 3, 2, 1, 5.0, 1e-5, None, False),
    "n64_t3": (4, 3, 3, 1, 0.0, 1e-5, None, True),
    "n64_t17_b5": (4, 3, 17, 5, 5.0, 1e-5, [1, 17, 5, 2, 16], True),
    "n125_t17_b5": (5, 3, 17, 5, 0.0, 1e-5, [17, 1, 3, 17, 9], True),
    "n125_t300": (5, 3, 300, 1, 1e4, 1e-5, None, True),
    "n256_t300": (4, 4, 300, 1, 0.0, 1e-5, None, True),
    "n256_t17_pen": (4, 4, 17, 1, 1e4, 1e-5, None, False),
    "n1024_t17_b5": (4, 5, 17, 5, 5.0, 1e-5, None, False),
    "n1024_t800": (4, 5, 800, 1, 0.0, 1e-5, None, True),
    "n64_zeros": (4, 3, 8, 1, 0.0, 0.0, None, None),
}


def case_post(name):
    nbase, klen, T, B, skip, mp, lens, sharp = CASES[name]
    if name == "n64_zeros":
        return zero_post()
    post = make_post(9000 + sorted(CASES).index(name), T, B, nbase ** klen + 1, sharp)
    if name == "n1024_t17_b5":
        post[5, 2, 1:400] = 0.0                             # exact zeros under a floor: prepare_post lifts them to min_prob
    return post


def run(post, nbase, klen, skip, mp, lens=None, gamma=True, mode=None, ws_short=0):
    """slk_viterbi_marginals_f32 on a host posterior [T, B, S] -> (rc, dict of host arrays)."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    T, B, S = post.shape
    N = S - 1
    pd = dev(post)
    need = int(L.slk_viterbi_marginals_workspace_bytes(T, B, nbase, klen))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    out = {"score": dev(np.full(B, SENT_F)), "path": dev(np.full((B, T), SENT_I)), "len": dev(np.full(B, SENT_I)),
           "move_row": dev(np.full((B, T), SENT_I)), "conf": dev(np.full((B, T), SENT_D)), "logz": dev(np.full(B, SENT_D))}
    if gamma:
        out["gamma"] = dev(np.full((T, B, max(N, 1)), SENT_F))
    ld = None if lens is None else dev(np.asarray(lens, dtype=np.int32))
    rc = L.slk_viterbi_marginals_f32(pd.data_ptr(), T, B, nbase, klen, float(skip), _lib.POST_RAW if mode is None else mode, float(mp),
                                     None if ld is None else ld.data_ptr(), ws.data_ptr(), max(need - ws_short, 0),
                                     out["score"].data_ptr(), out["path"].data_ptr(), out["len"].data_ptr(), out["move_row"].data_ptr(),
                                     out["conf"].data_ptr(), out["logz"].data_ptr(), out["gamma"].data_ptr() if gamma else None, stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def untouched(out):
    return all((v == {np.dtype(np.float32): SENT_F, np.dtype(np.int32): SENT_I, np.dtype(np.float64): SENT_D}[v.dtype]).all()
               for v in out.values())


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def device_transforms(post, mp):
    """(slk_prepare_post_f32's values, slk_log_post_f32's values) of a host posterior, as float32 host arrays."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    pd = dev(post)
    p, lp = torch.empty_like(pd), torch.empty_like(pd)
    assert L.slk_prepare_post_f32(pd.data_ptr(), p.data_ptr(), pd.numel(), float(mp), stream()) == 0
    assert L.slk_log_post_f32(pd.data_ptr(), lp.data_ptr(), pd.numel(), _lib.POST_RAW, float(mp), stream()) == 0
    return p.cpu().numpy(), lp.cpu().numpy()


@pytest.fixture(scope="module")
def results():
    """Per case: the device's outputs (with gamma), and per chunk the oracle in np.longdouble (the truth) and in float64 on the device's
    own prepared posterior and log-posterior.  E_m: the float64 oracle's largest distance from the truth."""
    out, e_m = {}, 0.0
    for name, (nbase, klen, T, B, skip, mp, lens, _) in CASES.items():
        post = case_post(name)
        rc, got = run(post, nbase, klen, skip, mp, lens)
        assert rc == 0, name
        p, lp = device_transforms(post, mp)
        chunks = []
        for b in range(B):
            n = T if lens is None else lens[b]
            score, path, rows = lr.viterbi(lp[:n, b], klen, skip, nbase)
            g_ld, z_ld = lr.marginals(p[:n, b], klen, skip, nbase, dtype=LD)
            g_64, z_64 = lr.marginals(p[:n, b], klen, skip, nbase)
            c_ld, c_64 = lr.confidence(g_ld, path, rows), lr.confidence(g_64, path, rows)
            e_m = max(e_m, float(np.abs(g_64 - g_ld).max()), float(np.abs(c_64 - c_ld).max()), abs(float(z_64 - z_ld)) / n)
            chunks.append({"n": n, "score": score, "path": path, "rows": rows, "gamma": g_ld, "logz": z_ld, "conf": c_ld, "p": p[:n, b]})
        out[name] = (post, got, chunks)
    print("E_m = %.3e" % e_m)
    assert 0.0 < e_m < 1e-12                               # a float64 recursion's distance from the exact value, not a tolerance
    out["E_m"] = e_m
    return out


# ---- 1: the bits of the existing decoder ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_decoder(results, name):
    """score_out, path_out and len_out are slk_viterbi_kmer_f32's on the same rows (a ragged chunk: on its own rows alone); move_row and
    the path are the numpy Viterbi's on the device's own log-posteriors.  Nothing is excluded."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    nbase, klen, T, B, skip, mp, lens, _ = CASES[name]
    post, got, chunks = results[name]
    for b, ch in enumerate(chunks):
        n = ch["n"]
        sub = dev(np.ascontiguousarray(post[:n, b:b + 1]))
        need = int(L.slk_viterbi_kmer_workspace_bytes(n, 1, nbase, klen))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        sc, pa, le = dev(np.zeros(1, np.float32)), dev(np.zeros((1, n), np.int32)), dev(np.zeros(1, np.int32))
        assert L.slk_viterbi_kmer_f32(sub.data_ptr(), n, 1, nbase, klen, float(skip), _lib.POST_RAW, float(mp), ws.data_ptr(), need,
                                      sc.data_ptr(), pa.data_ptr(), le.data_ptr(), stream()) == 0
        k = int(le.cpu().numpy()[0])
        assert int(got["len"][b]) == k == len(ch["path"]), (name, b)
        assert same(got["score"][b:b + 1], sc.cpu().numpy()) and float(got["score"][b]) == float(ch["score"]), (name, b)
        assert got["path"][b, :k].tolist() == pa.cpu().numpy()[0, :k].tolist() == ch["path"], (name, b)
        assert got["move_row"][b, :k].tolist() == ch["rows"], (name, b)
        assert (got["path"][b, k:] == -1).all() and (got["move_row"][b, k:] == -1).all() and (got["conf"][b, k:] == 0.0).all(), (name, b)


# ---- 2: accuracy of the float64 outputs ---------------------------------------------------------------------------------------------

def test_accuracy(results):
    """conf, log Z / T and gamma against the np.longdouble oracle: at most 4 E_m away (gamma: + 2^-24 gamma).
    Measured on an MI355X (one run): E_m 2.489e-15; conf 1.05 E_m, log Z / T 0.19 E_m, gamma 0.00 E_m beyond its rounding."""
    e_m = results["E_m"]
    worst = {"conf": 0.0, "logz": 0.0, "gamma": 0.0}
    for name in CASES:
        _, got, chunks = results[name]
        for b, ch in enumerate(chunks):
            n, k = ch["n"], len(ch["path"])
            d_conf = float(np.abs(got["conf"][b, :k].astype(LD) - ch["conf"]).max())
            d_logz = abs(float(LD(got["logz"][b]) - ch["logz"])) / n
            excess = np.abs(got["gamma"][:n, b].astype(LD) - ch["gamma"]) - LD(2.0 ** -24) * ch["gamma"]
            d_gamma = max(float(excess.max()), 0.0)
            worst = {"conf": max(worst["conf"], d_conf), "logz": max(worst["logz"], d_logz), "gamma": max(worst["gamma"], d_gamma)}
            print("%-14s chunk %d: conf %.2f E_m, logz/T %.2f E_m, gamma %.2f E_m" % (name, b, d_conf / e_m, d_logz / e_m, d_gamma / e_m))
            assert np.isfinite(got["logz"][b]) and np.isfinite(got["conf"][b]).all() and np.isfinite(got["gamma"][:, b]).all()
    print("E_m %.3e; largest device distances in E_m: %s" % (e_m, {k: round(v / e_m, 3) for k, v in worst.items()}))
    assert worst["conf"] <= ALLOW * e_m and worst["logz"] <= ALLOW * e_m and worst["gamma"] <= ALLOW * e_m, worst


def test_long_sharp_rows_do_not_underflow(results):
    """300 and 800 sharp rows with min_prob 1e-5: log Z is far below the float64 range of an unscaled product."""
    for name in ("n256_t300", "n125_t300", "n1024_t800"):
        _, got, chunks = results[name]
        assert got["logz"][0] < -2.0 * CASES[name][2] and chunks[0]["logz"] < -2.0 * CASES[name][2]
        assert (got["conf"][0, :int(got["len"][0])] > 0.0).all()


def test_exact_zero_on_the_called_path(results):
    """min_prob 0, exact zeros: the position that crosses the all-but-zero row has confidence exactly 0, Phred 0."""
    from sloika_amd import bio
    post, got, chunks = results["n64_zeros"]
    ch = chunks[0]
    k = int(got["len"][0])
    hit = [j for j in range(k) if ch["rows"][j] == 3]
    assert len(hit) == 1 and ch["p"][3, 1 + ch["path"][hit[0]]] == 0.0 and ch["p"][3, 0] == 0.0
    assert got["conf"][0, hit[0]] == 0.0 and ch["conf"][hit[0]] == 0.0
    assert (np.delete(got["conf"][0, :k], hit[0]) > 0.0).all() and k == 3
    assert bio.phred_of_error(1.0 - got["conf"][0, :k])[hit[0]] == 0


# ---- 3: structure -------------------------------------------------------------------------------------------------------------------

def test_structure(results):
    """Rows of gamma sum to 1 within N 2^-24; rows behind a chunk are 0; conf is at least the marginal at the row the position is entered
    (compared after the same rounding to float32)."""
    for name, (nbase, klen, T, B, skip, mp, lens, _) in CASES.items():
        _, got, chunks = results[name]
        N = nbase ** klen
        for b, ch in enumerate(chunks):
            n, k = ch["n"], len(ch["path"])
            g = got["gamma"][:, b]
            assert (g[:n] >= 0.0).all() and (g[n:] == 0.0).all(), (name, b)
            assert float(np.abs(g[:n].astype(np.float64).sum(axis=1) - 1.0).max()) <= N * 2.0 ** -24, (name, b)
            conf = got["conf"][b, :k]
            assert (conf >= 0.0).all() and (conf <= 1.0 + 1e-12).all()
            at_entry = g[got["move_row"][b, :k], got["path"][b, :k]]
            assert (conf.astype(np.float32) >= at_entry).all(), (name, b)
            ends = list(got["move_row"][b, 1:k]) + [n]
            dwell_max = np.array([g[r0:r1, s].max() for s, r0, r1 in zip(got["path"][b, :k], got["move_row"][b, :k], ends)])
            assert same(conf.astype(np.float32), dwell_max), (name, b)


@pytest.mark.parametrize("name", ["n64_t17_b5", "n125_t17_b5", "n1024_t17_b5"])
def test_same_bits_alone_in_a_batch_and_without_gamma(results, name):
    nbase, klen, T, B, skip, mp, lens, _ = CASES[name]
    post, got, chunks = results[name]
    rc, bare = run(post, nbase, klen, skip, mp, lens, gamma=False)
    assert rc == 0
    for key in ("score", "path", "len", "move_row", "conf", "logz"):
        assert same(bare[key], got[key]), key
    for b in (0, B - 1, 2):
        n = chunks[b]["n"]
        rc, one = run(np.ascontiguousarray(post[:n, b:b + 1]), nbase, klen, skip, mp, None)
        assert rc == 0
        for key in ("score", "len", "logz"):
            assert same(one[key], got[key][b:b + 1]), (key, b)
        for key in ("path", "move_row", "conf"):
            assert same(one[key][0], got[key][b, :n]), (key, b)
        assert same(one["gamma"][:, 0], got["gamma"][:n, b]), b
        # ... and with its rows given as a length of a longer chunk
        rc, rag = run(np.ascontiguousarray(post[:, b:b + 1]), nbase, klen, skip, mp, [n])
        assert rc == 0 and same(rag["conf"], got["conf"][b:b + 1]) and same(rag["gamma"][:, 0], got["gamma"][:, b])


def test_lengths_are_clamped():
    post = make_post(77, 6, 3, 65, False)
    rc, a = run(post, 4, 3, 0.0, 1e-5, [0, 9, -4])
    rc2, b = run(post, 4, 3, 0.0, 1e-5, [1, 6, 1])
    assert rc == 0 and rc2 == 0 and all(same(a[k], b[k]) for k in a)


def test_refusals_write_nothing():
    from sloika_amd import _lib
    L = _lib.lib()
    assert L.slk_viterbi_marginals_workspace_bytes(800, 1024, 4, 5) == 256 * ((800 * 1024 * (9 * 1024 + 20) + 255) // 256)
    for shape in ((10, 2, 4, 2), (10, 2, 4, 6), (10, 2, 5, 5), (10, 2, 3, 3), (10, 2, 2, 3), (0, 2, 4, 3), (10, 0, 4, 3)):
        assert L.slk_viterbi_marginals_workspace_bytes(*shape) == 0, shape
    post = make_post(5, 10, 2, 65, False)
    for nbase, klen, S in ((4, 2, 17), (4, 6, 4097), (5, 5, 3126), (3, 3, 28), (2, 3, 9)):
        rc, out = run(make_post(5, 4, 2, S, False), nbase, klen, 0.0, 1e-5)
        assert rc == _lib.SLK_ERR_UNSUPPORTED and untouched(out), (nbase, klen)
    for mode in (_lib.POST_LOG, _lib.POST_LN):
        rc, out = run(post, 4, 3, 0.0, 1e-5, mode=mode)
        assert rc == _lib.SLK_ERR_UNSUPPORTED and untouched(out)
    rc, out = run(post, 4, 3, 0.0, 1e-5, mode=7)
    assert rc == _lib.SLK_ERR_INVALID_ARG and untouched(out)
    rc, out = run(post, 4, 3, 0.0, 1.0)
    assert rc == _lib.SLK_ERR_INVALID_ARG and untouched(out)
    rc, out = run(post, 4, 3, 0.0, 1e-5, ws_short=1)
    assert rc == _lib.SLK_ERR_WORKSPACE and untouched(out)
    rc, out = run(post, 4, 3, 0.0, 1e-5, mode=_lib.POST_PLAIN)
    assert rc == 0 and not untouched(out)


def test_plain_mode_takes_the_posterior_as_it_is():
    post = make_post(6, 9, 2, 65, True)
    rc, raw0 = run(post, 4, 3, 0.7, 0.0)
    from sloika_amd import _lib
    rc2, plain = run(post, 4, 3, 0.7, 0.0, mode=_lib.POST_PLAIN)
    assert rc == 0 and rc2 == 0 and all(same(raw0[k], plain[k]) for k in raw0)


# ---- 4: bases with qualities --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("klen,always_move", [(3, 1), (3, 0), (5, 1), (5, 0)])
def test_bases_with_qualities(klen, always_move):
    """Letters and counts are slk_paths_to_bases' byte for byte; a letter's quality is the search of the host's table for 1 - conf of
    the position that emitted it.  A repeated state, cap exactly klen * max(lens), a conf that is NaN."""
    torch = need_gpu()
    from sloika_amd import _lib, bio
    L = _lib.lib()
    rs = np.random.RandomState(40 + klen)
    N, B, T = 4 ** klen, 4, 300
    lens = np.array([300, 1, 257, 0], dtype=np.int32)
    paths = rs.randint(0, N, size=(B, T)).astype(np.int32)
    for i in range(1, T):                                   # mostly single steps, some repeats
        step = (paths[:, i - 1] % (N // 4)) * 4 + rs.randint(0, 4, size=B)
        paths[:, i] = np.where(rs.rand(B) < 0.7, step, paths[:, i])
    paths[0, 5] = paths[0, 4]
    paths[2, 256] = paths[2, 255]
    conf = 1.0 - 10.0 ** (-rs.uniform(0, 7.5, size=(B, T)))
    conf[0, :8] = [0.0, 1.0, 0.9, np.nextafter(0.9, 1), np.nextafter(0.9, 0), np.nan, 0.5, 1.0 - 1e-6]
    qmax = 60
    cap = klen * int(lens.max())
    pd, ld, cd, td = dev(paths), dev(lens), dev(conf), dev(bio.phred_thresholds(qmax))
    packed = int.from_bytes(b"ACGT".ljust(8, b"\0"), "little")
    o1, n1 = torch.zeros((B, cap), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    o2, q2, n2 = torch.zeros_like(o1), torch.full_like(o1, 255), torch.zeros_like(n1)
    assert L.slk_paths_to_bases(pd.data_ptr(), T, ld.data_ptr(), B, klen, 4, always_move, packed, o1.data_ptr(), cap, n1.data_ptr(),
                                stream()) == 0
    assert L.slk_paths_to_bases_qual(pd.data_ptr(), T, ld.data_ptr(), cd.data_ptr(), T, td.data_ptr(), qmax, B, klen, 4, always_move,
                                     packed, o2.data_ptr(), q2.data_ptr(), cap, n2.data_ptr(), stream()) == 0
    o1, n1, o2, q2, n2 = (t.cpu().numpy() for t in (o1, n1, o2, q2, n2))
    assert same(n1, n2) and same(o1, o2)
    assert n1[0] > klen and n1[1] == klen and n1[3] == 0
    for b in range(B):
        if lens[b] < 1:
            continue
        moves = bio.moves_of_states(paths[b, :lens[b]], klen, 4, allow_identical=not always_move)
        take = np.concatenate(([klen], np.minimum(moves, klen)))
        want = np.repeat(bio.phred_of_error(1.0 - conf[b, :lens[b]], qmax), take).astype(np.uint8)
        assert len(want) == n2[b] and same(q2[b, :n2[b]], want), b
        assert (q2[b, n2[b]:] == 255).all()
    if not always_move:
        assert n1[0] < klen + (lens[0] - 1) * klen             # the repeated states emitted nothing
    assert q2[0, 0] == 0 and q2[0, klen - 1] == 0               # conf 0 -> Phred 0 on all klen letters of the first position
    bad = L.slk_paths_to_bases_qual(pd.data_ptr(), T, ld.data_ptr(), cd.data_ptr(), T, td.data_ptr(), 94, B, klen, 4, always_move,
                                    packed, torch.zeros(1).data_ptr(), torch.zeros(1).data_ptr(), cap, dev(n2).data_ptr(), stream())
    assert bad == _lib.SLK_ERR_INVALID_ARG


# ---- 5: the pipeline ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_model():
    need_gpu()
    from sloika_amd import models
    return models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=7))


def test_call_chunks_qual_is_the_unfused_decoder(small_model):
    from sloika_amd import decode, pipeline
    chunks = pipeline.synthetic_chunks(3, chunk_len=400, seed=5)
    bc = pipeline.Basecaller(small_model, kmer_len=5, skip=5.0, fused_decode=False)
    s0, p0, l0 = (t.cpu().numpy() for t in bc.call_chunks(chunks))
    res = pipeline.Basecaller(small_model, kmer_len=5, skip=5.0).call_chunks_qual(chunks)
    s1, p1, l1, rows, conf, logz = (t.cpu().numpy() for t in res)
    assert same(s0, s1) and same(p0, p1) and same(l0, l1)
    assert conf.dtype == np.float64 and logz.dtype == np.float64 and np.isfinite(logz).all()
    for b in range(3):
        k = l1[b]
        assert rows[b, 0] == 0 and (np.diff(rows[b, :k]) > 0).all() and ((conf[b, :k] > 0) & (conf[b, :k] <= 1.0 + 1e-12)).all()
    # a split of the batch over several launches changes nothing
    post = bc.posteriors(chunks)
    whole = decode.viterbi_marginals_batch(post, 5, skip_pen=5.0, gamma=True)
    alone = int(decode._lib.lib().slk_viterbi_marginals_workspace_bytes(post.shape[0], 1, 4, 5))
    split = decode.viterbi_marginals_batch(post, 5, skip_pen=5.0, gamma=True, workspace_limit=2 * alone)
    assert all(same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(whole, split))
    assert same(whole[4].cpu().numpy(), conf)
    with pytest.raises(ValueError):
        decode.viterbi_marginals_batch(post, 5, workspace_limit=alone - 1)
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller(small_model, kmer_len=5, transducer=False).call_chunks_qual(chunks)


def test_call_reads_qual_and_fastq(small_model):
    from sloika_amd import bio, pipeline
    base = pipeline.synthetic_chunks(3, chunk_len=1500, seed=21)
    reads = [base[0], base[1][:700], base[2][:1130]]
    bc = pipeline.Basecaller(small_model, kmer_len=5, skip=0.0)
    res = bc.call_reads_qual(reads)
    nsamp = res[-1]
    got = [t.cpu().numpy() for t in res[:-1]]
    ref = [t.cpu().numpy() for t in pipeline.Basecaller(small_model, kmer_len=5, skip=0.0, fused_decode=False).call_reads(reads)[:3]]
    assert same(got[0], ref[0]) and same(got[1], ref[1]) and same(got[2], ref[2])
    for b, r in enumerate(reads):
        one = bc.call_reads_qual([r])
        assert one[-1][0] == nsamp[b]
        k = int(got[2][b])
        for key in (0, 2, 5):
            assert same(one[key].cpu().numpy(), got[key][b:b + 1]), (b, key)
        for key in (1, 3, 4):
            assert same(one[key].cpu().numpy()[0, :k], got[key][b, :k]), (b, key)
    calls = bio.paths_to_bases_qual(res[1], res[2], res[4], 5)
    plain = bio.paths_to_bases(res[1], res[2], 5)
    records = bc.call_fastq(reads, names=["a", "b", "c"])
    assert len(records) == 3
    for b, rec in enumerate(records):
        head, seq, plus, qual, rest = rec.split("\n")
        assert head == "@" + "abc"[b] and plus == "+" and rest == ""
        assert seq == calls[b][0] == plain[b] and len(qual) == len(seq)
        q = np.frombuffer(qual.encode(), dtype=np.uint8) - 33
        assert same(q.astype(np.uint8), calls[b][1]) and q.max() <= 60
        k = int(got[2][b])
        want = np.repeat(bio.phred_of_error(1.0 - got[4][b, :k]), np.concatenate(([5], np.minimum(bio.moves_of_states(got[1][b, :k], 5, 4, False), 5))))
        assert same(calls[b][1], want.astype(np.uint8))
