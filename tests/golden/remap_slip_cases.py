"""The seeded inputs behind tests/golden/remap_slips.npz: reads whose best mapping SLIPS over many reference positions, so that the
remap DP (transducer.map_to_sequence; csrc/transducer.hip) leaves the easy side of its slip scan, its arg-max and its backtrace
window.  Shared by the generator (make_remap_slip_goldens.py) and by both test files; plain numpy, nothing here touches the
reference or a GPU.

Inputs are log-space rows already (`log=True` everywhere), drawn from RandomState.random_sample / randint and rounded to a grid:
no transcendental is evaluated, so the same bits come out of every numpy build and every score can be compared bit for bit.

A *planted path* input puts the largest value of every event on the k-mer of the planted position when the path moves there,
on blank (state 0) when it stays; every other state sits `contrast` lower.  A jump costs `slip` per position skipped, and the
cheapest way round a jump is a run of mismatched events, so `contrast` is chosen per case to keep the planted jump the best
move.  The positions on both sides of a planted jump carry states that occur nowhere else in the sequence: a jump can then not
be split into two shorter ones at the same total cost.  What the DP really decodes is recorded by the reference in the
fixture; every case names in `needs` the property that path must show, and `unmet(...)` checks it."""
import hashlib

import numpy as np

JUMP_LENGTHS = (2, 3, 62, 63, 64, 65, 127, 128, 129, 200, 700)
BATCH_ROWS = 32                     # events per round trip of the device's backtrace
WINDOW = 64                         # traceback entries it holds per event: positions cur-63 .. cur


def sha256_hex(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def plant_path(rs, nev, npos, jumps, start=0, end=None, all_step=False):
    """int64 [nev]: starts at `start`, jumps by `length` at every (event, length) of `jumps`, steps by one at randomly chosen
    other events so as to finish at `end` (default: the last position), stays elsewhere.  The events next to a jump stay where
    there is room for it."""
    jump_at = dict((int(e), int(n)) for e, n in jumps)
    assert all(1 <= e < nev for e in jump_at), "a jump needs an event to happen in"
    end = npos - 1 if end is None else end
    near = set()
    for e in jump_at:
        near.update((e - 1, e + 1))
    free = [t for t in range(1, nev) if t not in jump_at and (all_step or t not in near)]
    nstep = int(np.clip(end - start - sum(jump_at.values()), 0, len(free)))
    move = np.zeros(nev, dtype=np.int64)
    if nstep:
        move[rs.choice(free, size=nstep, replace=False)] = 1
    for e, n in jump_at.items():
        move[e] = n
    path = start + np.cumsum(move)
    assert path[-1] < npos, "the planted path leaves the sequence"
    return path


def planted(seed, nev, npos, nst, jumps=(), start=0, end=None, all_step=False, contrast=8.0, grid=1024.0, spread=2.0,
            neginf=0.0, blocked=()):
    """-> (ltrans float32 [nev, nst], sequence int32 [npos], planted path int64 [nev]).

    grid    : every value is a multiple of 1/grid (grid=4: the quantised variant, stay / step / slip tie exactly and often)
    neginf  : fraction of the off-path (event, k-mer) entries that are impossible (-inf)
    blocked : events at which the planted k-mer itself is impossible, so the best path has to leave the planted one"""
    rs = np.random.RandomState(seed)
    path = plant_path(rs, nev, npos, jumps, start, end, all_step)
    special = sorted(set(int(path[e - 1]) for e, _ in jumps) | set(int(path[e]) for e, _ in jumps))
    assert len(special) + 2 < nst, "not enough k-mers to give every jump its own"
    seq = rs.randint(1 + len(special), nst, size=npos).astype(np.int32)
    seq[special] = 1 + np.arange(len(special), dtype=np.int32)
    lt = -contrast - spread * rs.random_sample((nev, nst))
    moved = np.ones(nev, dtype=bool)
    moved[1:] = np.diff(path) != 0
    target = np.where(moved, seq[path], 0)
    if neginf > 0.0:
        lt[rs.random_sample((nev, nst)) < neginf] = -np.inf
    lt[np.arange(nev), target] = -0.25 * rs.random_sample(nev)
    for e in blocked:
        lt[e, target[e]] = -np.inf
    with np.errstate(invalid="ignore"):
        lt = np.round(lt * grid) / grid
    return lt.astype(np.float32), seq, path


def priors(seed, npos, initial, final):
    """float64 priors with all 53 bits in use and magnitudes from 1e-3 to 1e5: the float64 add and its one rounding to float32
    differ from a float32 add of the rounded prior."""
    rs = np.random.RandomState(seed)
    def one():
        return -(rs.random_sample(npos) * 10.0 ** rs.randint(-3, 6, size=npos))
    pi = one() if initial else None
    pf = one() if final else None
    return pi, pf


# ---- a numpy float32 restatement of the forward pass (small cases only: the slip recurrence is a Python loop) -------------------------

def slip_update_np(x, slip):
    n = len(x)
    fs = np.full(n, np.float32(-1e38), dtype=np.float32)
    fp = np.zeros(n, dtype=np.int64)
    c, p = np.float32(-np.inf), 0
    for k in range(n - 2):
        if not c >= x[k]:
            c, p = x[k], k
        c = np.float32(c - slip)
        fs[k + 2], fp[k + 2] = c, p
    return fs, fp


def forward_np(lt, seq, slip, prior_initial=None, upto=None):
    """Scores over the positions after event `upto` - 1 (default: all events), before prior_final: float32 [npos]."""
    slip = np.float32(slip)
    ps = np.zeros(len(seq), dtype=np.float32)
    if prior_initial is not None:
        ps = (ps.astype(np.float64) + prior_initial).astype(np.float32)
    ps = ps + np.fmax(lt[0][seq], lt[0][0])
    for i in range(1, len(lt) if upto is None else upto):
        ps = candidates_np(ps, lt[i], seq, slip).max(axis=0)
    return ps


def candidates_np(ps, row, seq, slip):
    """float32 [3, npos]: the stay, step and slip candidates of one event from the scores `ps` before it."""
    stay = ps + row[0]
    step = np.full(len(ps), -np.inf, dtype=np.float32)
    step[1:] = ps[:-1] + row[seq[1:]]
    fs, _ = slip_update_np(ps, np.float32(slip))
    return np.stack([stay, step, fs + row[seq]])


def tying_prior_final(lt, seq, slip, gap):
    """A float64 prior over the final position that makes exactly two positions, `gap` apart, share the best final score.  For
    the quantised inputs every score is a small multiple of 1/4, so the float64 sum is exact."""
    ps = forward_np(lt, seq, slip)
    hi = int(np.argmax(np.where(np.arange(len(ps)) >= gap, ps, -np.inf)))
    lo = hi - gap
    assert np.isfinite(ps[hi]) and np.isfinite(ps[lo])
    pf = np.full(len(ps), -1000.0)
    pf[hi] = 0.0
    pf[lo] = float(ps[hi]) - float(ps[lo])
    return pf


# ---- the device's backtrace, restated on a finished path ------------------------------------------------------------------------------

def backtrace_batches(path):
    """How csrc/transducer.hip walks back along `path`: from the current position it holds positions cur-63 .. cur (never below
    0) of up to BATCH_ROWS events; a move below the window ends the batch at that row.  -> list of (rows done, jump) for every
    batch that a move out of its window ended; rows done = 1: the move sat on the batch's first row."""
    out = []
    r = len(path) - 1
    while r >= 1:
        cur = int(path[r])
        base = max(cur - (WINDOW - 1), 0)
        done = 0
        for l in range(BATCH_ROWS):
            if r - l < 1:
                break
            prev = int(path[r - l - 1])
            done = l + 1
            if prev < base:
                out.append((done, int(path[r - l]) - prev))
                break
        r -= done
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------

def _spaced(lengths, first, gap):
    return [(first + gap * i, n) for i, n in enumerate(lengths)]


def _case(slip, needs, pri=(False, False), tie_gap=None, **gen):
    return dict(slip=slip, needs=needs, pri=pri, tie_gap=tie_gap, gen=gen)


CASES = {}

# every listed jump length in one read; eleven jumps 37 events apart, so they fall on different rows of the backtrace's batches
for _nst in (65, 1025):
    for _slip, _contrast in ((5.0, 512.0), (0.0, 8.0), (37.25, 4096.0)):
        CASES["jumps_n%d_s%g" % (_nst, _slip)] = _case(
            _slip, dict(jumps=JUMP_LENGTHS), seed=len(CASES) + 1, nev=430, npos=2100, nst=_nst,
            jumps=_spaced(JUMP_LENGTHS, 20, 37), contrast=_contrast)

# the backtrace's batches, counted back from the last event: a move out of the window on the first, second, last-but-one and last
# row of a batch; two in one batch; in consecutive events; and one that leaves the window only because the path had already
# stepped down through most of it
for _name, _jumps, _needs, _extra in (
        ("bt_first", [(99, 100)], dict(jumps=[100], ends=[1]), {}),
        ("bt_second", [(98, 100)], dict(jumps=[100], ends=[2]), {}),
        ("bt_last_but_one", [(69, 100)], dict(jumps=[100], ends=[31]), {}),
        ("bt_last", [(68, 100)], dict(jumps=[100], ends=[32]), {}),
        ("bt_two_in_batch", [(95, 90), (80, 80)], dict(jumps=[80, 90], ends=[5]), {}),
        ("bt_consecutive", [(50, 70), (51, 66), (52, 64)], dict(jumps=[64, 66, 70], ends=[1]), {}),
        ("bt_drift", [(75, 40)], dict(jumps=[40], short_end=True), dict(all_step=True, end=199))):
    CASES[_name] = _case(5.0, _needs, seed=len(CASES) + 1, nev=100, npos=400, nst=65, jumps=_jumps, contrast=1024.0, **_extra)

# the window's edges
CASES["edge_base0"] = _case(5.0, dict(jumps=[40], jump_from_below=63), seed=len(CASES) + 1, nev=60, npos=300, nst=65,
                            jumps=[(10, 40)], start=5, end=70, contrast=64.0)
CASES["edge_land0"] = _case(5.0, dict(jumps=[100], lands_on_zero=True), seed=len(CASES) + 1, nev=60, npos=300, nst=65,
                            jumps=[(1, 100)], start=0, contrast=1024.0)
CASES["edge_tail"] = _case(5.0, dict(jumps=[90], ends_in_tail=3), seed=len(CASES) + 1, nev=60, npos=300, nst=65,
                           jumps=[(57, 90)], start=153, contrast=1024.0)
CASES["edge_small"] = _case(5.0, dict(jumps=[20, 9]), seed=len(CASES) + 1, nev=50, npos=40, nst=65,
                            jumps=[(12, 20), (30, 9)], contrast=256.0)

# event counts round the batch length; positions round every change of the scan's segment length and of the LDS request
for _nev in (1, 2, 3, 31, 32, 33, 34, 64, 65, 97):
    CASES["nev_%d" % _nev] = _case(
        5.0, dict(jumps=[70]) if _nev > 1 else {}, seed=len(CASES) + 1, nev=_nev, npos=150, nst=65,
        jumps=[(max(1, _nev // 2), 70)] if _nev > 1 else [], start=3, contrast=512.0)
for _npos in (3, 4, 5, 65, 66, 67, 129, 130, 131, 194, 195):
    _j = _npos - 1                                      # position 0 to the last one: the scan's chain walks the whole array
    CASES["npos_%d" % _npos] = _case(
        (0.0, 5.0)[_npos % 2], dict(jumps=[_j]), seed=len(CASES) + 1, nev=40, npos=_npos, nst=65, jumps=[(20, _j)],
        contrast=8.0 * _npos)
for _npos in (2336, 2337):
    CASES["npos_%d" % _npos] = _case(
        5.0, dict(jumps=[700, _npos - 1001]), seed=len(CASES) + 1, nev=97, npos=_npos, nst=1025,
        jumps=[(30, 700), (70, _npos - 1001)], start=210, contrast=8192.0)
CASES["npos_5846"] = _case(5.0, dict(jumps=[700, 3000, 64]), seed=len(CASES) + 1, nev=2000, npos=5846, nst=1025,
                           jumps=[(400, 700), (1000, 3000), (1969, 64)], start=91, contrast=2048.0)

# impossible k-mers
CASES["neginf_n65"] = _case(5.0, dict(jumps=[64, 129], finite=True), seed=len(CASES) + 1, nev=120, npos=500, nst=65,
                            jumps=[(40, 64), (80, 129)], contrast=64.0, neginf=0.3, blocked=(10, 11, 60, 100))
CASES["neginf_n1025"] = _case(0.0, dict(jumps=[200], finite=True), seed=len(CASES) + 1, nev=120, npos=500, nst=1025,
                              jumps=[(50, 200)], contrast=16.0, neginf=0.3, blocked=(20, 70, 71))

# the quantised variant (values 0, -1/4, -1/2, ...): stay, step and slip tie exactly on the decoded path; then the same with a
# prior_final that makes two final positions, more than 64 apart, share the best score (the earlier one on the lower lane of the
# device's arg-max in two cases, on the higher lane in the third)
for _name, _slip, _gap, _gen in (("200", 0.0, 100, dict(seed=52, nev=60, npos=200, jumps=[(30, 70)], spread=0.25)),
                                 ("1000", 0.0, 411, dict(seed=50, nev=90, npos=1000, jumps=[(45, 70)], spread=0.25)),
                                 ("1000_s025", 0.25, 100, dict(seed=51, nev=90, npos=1000, jumps=[(45, 70)], spread=0.5))):
    CASES["quant_" + _name] = _case(_slip, dict(three_way_tie=True), nst=65, contrast=0.25, grid=4.0, **_gen)
    CASES["tie_" + _name] = _case(_slip, dict(final_tie=True), tie_gap=_gap, nst=65, contrast=0.25, grid=4.0, **_gen)

# priors
for _name, _pri in (("prior_initial", (True, False)), ("prior_final", (False, True)), ("prior_both", (True, True))):
    CASES[_name] = _case(5.0, dict(jumps=[65, 128]), pri=_pri, seed=len(CASES) + 1, nev=100, npos=450, nst=65,
                         jumps=[(30, 65), (66, 128)], start=20, end=430, contrast=4096.0)

NAMES = list(CASES)


def build(name):
    """-> dict(name, slip, ltrans, seq, pi, pf, planted, needs) of a named case."""
    c = CASES[name]
    lt, seq, path = planted(**c["gen"])
    pi, pf = priors(c["gen"]["seed"] + 5000, len(seq), *c["pri"])
    if c["tie_gap"] is not None:
        pf = tying_prior_final(lt, seq, c["slip"], c["tie_gap"])
    return dict(name=name, slip=c["slip"], ltrans=lt, seq=seq, pi=pi, pf=pf, planted=path, needs=c["needs"])


def digest(case):
    return sha256_hex(case["ltrans"], case["seq"], case["pi"], case["pf"])


def jumps_of(path):
    return np.diff(np.asarray(path, dtype=np.int64)) if len(path) > 1 else np.zeros(0, dtype=np.int64)


def unmet(case, path, score):
    """The `needs` of a case that `path` / `score` do NOT show (empty list: the case tests what it is there for)."""
    needs, miss = case["needs"], []
    d = jumps_of(path)
    for n in needs.get("jumps", ()):
        if not (d == n).any():
            miss.append("no jump of exactly %d" % n)
    ends = backtrace_batches(path)
    for rows in needs.get("ends", ()):
        if not any(done == rows and jump >= WINDOW for done, jump in ends):
            miss.append("no backtrace batch ended on row %d by a jump of a window or more" % rows)
    if needs.get("short_end") and not any(jump < WINDOW and done < BATCH_ROWS for done, jump in ends):
        miss.append("no batch ended early by a jump shorter than the window")
    if "jump_from_below" in needs and not ((d >= 2) & (np.asarray(path[1:]) < needs["jump_from_below"])).any():
        miss.append("no jump that starts below position %d" % needs["jump_from_below"])
    if needs.get("lands_on_zero") and not ((d >= 2) & (np.asarray(path[:-1]) == 0)).any():
        miss.append("no jump that lands on position 0")
    if "ends_in_tail" in needs and not path[-1] >= len(case["seq"]) - needs["ends_in_tail"]:
        miss.append("path does not end in the last %d positions" % needs["ends_in_tail"])
    if needs.get("finite"):
        lt, seq = case["ltrans"], case["seq"]
        em = np.where(np.concatenate([[True], d != 0]), lt[np.arange(len(path)), seq[path]], lt[:, 0])
        if not (np.isfinite(score) and np.isfinite(em).all() and not np.isfinite(lt).all()):
            miss.append("score or an emission on the path is not finite")
        if np.array_equal(path, case["planted"]):
            miss.append("the path did not have to leave the planted one")
    if needs.get("final_tie"):
        final = (forward_np(case["ltrans"], seq=case["seq"], slip=case["slip"], prior_initial=case["pi"]).astype(np.float64)
                 + case["pf"]).astype(np.float32)
        best = np.flatnonzero(final == final.max())
        if not (len(best) == 2 and best[1] - best[0] > WINDOW and path[-1] == best[0] and score == final.max()):
            miss.append("not exactly two best final positions more than 64 apart, the first of them taken")
    if needs.get("three_way_tie") and not three_way_ties(case, path):
        miss.append("stay, step and slip tie nowhere on the path")
    return miss


def three_way_ties(case, path):
    """Events at which stay, step and slip into the path's position tie exactly (recomputed in numpy float32)."""
    lt, seq, slip = case["ltrans"], case["seq"], case["slip"]
    ps = np.zeros(len(seq), dtype=np.float32)
    if case["pi"] is not None:
        ps = (ps.astype(np.float64) + case["pi"]).astype(np.float32)
    ps = ps + np.fmax(lt[0][seq], lt[0][0])
    found = []
    for i in range(1, len(lt)):
        cand = candidates_np(ps, lt[i], seq, slip)
        j = int(path[i])
        if j >= 2 and np.isfinite(cand[0, j]) and cand[0, j] == cand[1, j] == cand[2, j]:
            found.append(i)
        ps = cand.max(axis=0)
    return found


# ---- the sweep of tests/test_gpu_remap_slips.py ---------------------------------------------------------------------------------------

SWEEP_NPOS = list(range(3, 401)) + [1000, 2336, 2337, 4000, 5846]
SWEEP_NEV = (1, 2, 33, 257, 2000)
SWEEP_SLIP = (0.0, 2.5, 5.0)
SWEEP_NST = 65


def sweep_read(seed, nev, npos):
    """One planted read of the sweep: where the read is long enough, a jump of 64 or more (up to the whole sequence) and up to two
    shorter ones at random events."""
    rs = np.random.RandomState([seed, nev, npos])
    jumps = []
    if nev >= 2 and npos >= 70:
        events = rs.choice(np.arange(1, nev), size=min(3, nev - 1), replace=False)
        room = npos - 1
        for i, e in enumerate(sorted(int(v) for v in events)):
            n = int(rs.randint(64, min(room, 900) + 1)) if i == 0 else int(rs.randint(2, 64))
            if n <= room - 2:
                jumps.append((e, n))
                room -= n
    elif nev >= 2:
        jumps.append((int(rs.randint(1, nev)), int(rs.randint(2, npos))))
    return planted(int(rs.randint(1 << 30)), nev, npos, SWEEP_NST, jumps=jumps, contrast=6.0 * max(64, min(npos, 900)) / 8.0)


# ---- a whole read for chunkify_raw.raw_remap ---------------------------------------------------------------------------------------------

def skipping_read(seed=77, nbase=404, nstep=300, skip=100, stride=5):
    """-> (reference bytes, signal float32 [nstep * stride], posterior float32 [nstep, 1025]) of a read that skips `skip` bases of
    its reference in one place.  The posterior holds two values only (0.9 on the planted 5-mer or on blank, the rest shared
    evenly), so its logarithm does not depend on whose float32 log evaluates it."""
    rs = np.random.RandomState(seed)
    ref = bytes(rs.choice(list(b"ACGT"), size=nbase).tolist())
    digits = np.asarray([b"ACGT".index(c) for c in ref], dtype=np.int64)
    npos = nbase - 4
    states = 1 + sum(digits[j:j + npos] * 4 ** (4 - j) for j in range(5))
    path = plant_path(rs, nstep, npos, [(nstep // 2, skip)])
    moved = np.ones(nstep, dtype=bool)
    moved[1:] = np.diff(path) != 0
    post = np.full((nstep, 1025), 0.1 / 1024, dtype=np.float32)
    post[np.arange(nstep), np.where(moved, states[path], 0)] = np.float32(0.9)
    signal = (90.0 + 12.0 * rs.random_sample(nstep * stride)).astype(np.float32)
    return ref, signal, post
