"""The seeded inputs behind tests/golden/event_remap.npz: event reads with their references, and the posterior a network is taken
to have given for them, for `chunkify remap` of event models (sloika/batch.py:143-190).  Shared by the generator
(make_event_remap_goldens.py) and by both test files; plain numpy, nothing here touches the reference or a GPU.

The posterior of a case follows a *planted path* (remap_slip_cases.plant_path): at an event where the path moves, most of the mass
sits on the k-mer of the new position, where it stays, on blank; the rest is Dirichlet noise.  The margins are wide, so the remap's
path is not decided by the last bit of a float32 logarithm.  What the DP really decodes is recorded by the reference in the
fixture; every case names in `needs` what that path must show, and `unmet(...)` checks it -- in the generator, which refuses a case
that does not show it, and again in the tests."""
import hashlib

import numpy as np

import remap_slip_cases as rsc

ALPHABET = b"ACGT"
MIN_PROB = 1e-5

#: name -> kmer_len, events, reference bases, chunk_len, normalisation, use_scaled, prior, slip, planted jumps (event, length), needs
CASES = {
    # k = 5, a whole number of chunks of 100, both priors, a jump of 3 and one of 2
    "k5_cl100_exact": dict(seed=301, k=5, nev=700, nbase=330, chunk_len=100, normalisation="per-read", use_scaled=False,
                           prior=(25.0, 25.0), slip=5.0, jumps=[(250, 3), (520, 2)], needs=dict(jump=True, remainder=0)),
    # k = 5, three chunks of 100 and 33 events over; a stay on the first event of a chunk
    "k5_cl100_rest": dict(seed=302, k=5, nev=333, nbase=150, chunk_len=100, normalisation="per-chunk", use_scaled=True,
                          prior=(None, None), slip=5.0, jumps=[(160, 2)], needs=dict(jump=True, remainder=33, stay_on_chunk_start=True)),
    # k = 3, six chunks of 7 and 3 events over, no priors
    "k3_cl7_rest": dict(seed=303, k=3, nev=45, nbase=24, chunk_len=7, normalisation="per-chunk", use_scaled=False,
                        prior=(None, None), slip=5.0, jumps=[], needs=dict(remainder=3, stay_on_chunk_start=True)),
    # k = 3, seven chunks of 7 exactly, both priors
    "k3_cl7_exact": dict(seed=304, k=3, nev=49, nbase=30, chunk_len=7, normalisation="per-read", use_scaled=False,
                         prior=(25.0, 25.0), slip=2.5, jumps=[(20, 4)], needs=dict(jump=True, remainder=0)),
    # chunks of one event: every event is a chunk's first, so no label is ever zeroed; the path never moves after the first step
    "k3_cl1_all_stay": dict(seed=305, k=3, nev=20, nbase=12, chunk_len=1, normalisation="none", use_scaled=False,
                            prior=(None, None), slip=5.0, jumps=[], all_stay=True, needs=dict(all_stay=True, remainder=0)),
    # chunks of one event on a path that moves
    "k5_cl1_moving": dict(seed=306, k=5, nev=60, nbase=40, chunk_len=1, normalisation="per-read", use_scaled=False,
                          prior=(25.0, 25.0), slip=5.0, jumps=[(30, 2)], needs=dict(jump=True, remainder=0)),
}
NAMES = list(CASES)

TABLE_DTYPE = [("start", "f8"), ("length", "f8"), ("mean", "f8"), ("stdv", "f8"), ("scaled_mean", "f8"), ("scaled_stdv", "f8")]


def sha256_hex(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def states_of(ref, k):
    """state + 1 of every k-mer of `ref` (bio.all_kmers order: first letter most significant)."""
    digits = np.asarray([ALPHABET.index(c) for c in ref], dtype=np.int64)
    npos = len(ref) - k + 1
    return 1 + sum(digits[j:j + npos] * 4 ** (k - 1 - j) for j in range(k))


def build(name):
    """-> dict(name, k, ref bytes, ev (the event table: no 'kmer', 'seq_pos' or 'good_emission' column), post float32 [nev, 4^k + 1],
    planted int64 [nev], and the case's parameters)."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    k, nev, nbase = c["k"], c["nev"], c["nbase"]
    nst = 4 ** k + 1
    ref = bytes(rs.choice(list(ALPHABET), size=nbase).tolist())
    states = states_of(ref, k)
    npos = len(states)
    if c.get("all_stay"):
        planted = np.full(nev, npos // 2, dtype=np.int64)
    else:
        planted = rsc.plant_path(rs, nev, npos, c["jumps"])
    moved = np.ones(nev, dtype=bool)
    moved[1:] = np.diff(planted) != 0
    post = rs.dirichlet(np.ones(nst) * 0.05, size=nev)
    w = rs.uniform(0.6, 0.9, size=nev)
    post *= (1.0 - w)[:, None]
    post[np.arange(nev), np.where(moved, states[planted], 0)] += w
    post = (post / post.sum(axis=1, keepdims=True)).astype(np.float32)
    ev = np.zeros(nev, dtype=TABLE_DTYPE)
    level = rs.normal(size=npos)
    ev["mean"] = 90.0 + 12.0 * level[planted] + rs.normal(scale=0.8, size=nev)
    ev["stdv"] = np.abs(1.5 + 0.4 * rs.normal(size=nev))
    ev["length"] = (rs.geometric(0.1, size=nev) + 2) / 4000.0
    ev["start"] = np.concatenate([[0.0], np.cumsum(ev["length"])[:-1]])
    ev["scaled_mean"] = ev["mean"] * 1.03125 - 2.5
    ev["scaled_stdv"] = ev["stdv"] * 1.03125
    out = dict(c)
    out.update(name=name, ref=ref, states=states, ev=ev, post=post, planted=planted)
    return out


def digest(case):
    """One sha256 over everything the reference is handed for a case."""
    h = hashlib.sha256()
    h.update(case["ref"])
    for f, _ in TABLE_DTYPE:
        h.update(np.ascontiguousarray(case["ev"][f]).tobytes())
    h.update(np.ascontiguousarray(case["post"]).tobytes())
    return h.hexdigest()


def unmet(case, path):
    """The `needs` of a case that `path` does NOT show (empty list: the case tests what it is there for)."""
    needs, miss = case["needs"], []
    path = np.asarray(path, dtype=np.int64)
    d = np.diff(path)
    cl, nev = case["chunk_len"], len(path)
    if nev % cl != needs["remainder"]:
        miss.append("%d events leave %d over chunks of %d, not %d" % (nev, nev % cl, cl, needs["remainder"]))
    if needs.get("jump") and not (d >= 2).any():
        miss.append("no jump by 2 or more")
    if needs.get("stay_on_chunk_start"):
        first = np.arange(cl, (nev // cl) * cl, cl)
        if not (len(first) and (d[first - 1] == 0).any()):
            miss.append("no stay on the first event of a chunk")
    if needs.get("all_stay") and not (nev >= 3 and (d[1:] == 0).all()):
        miss.append("the path moves after the first step")
    return miss
