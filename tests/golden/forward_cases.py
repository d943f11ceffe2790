"""The seeded inputs behind tests/golden/forward.npz: (posterior, sequence) pairs for the forward score (decode.forwards,
csrc/forward_score.hip; design/forward_score.md).  Shared by the generator (make_forward_goldens.py) and both test files; plain
numpy, nothing here touches the reference or a GPU.

A posterior is built from exactly-rounded operations only (uniform draws, products, one boosted column per row, a division by
np.sum): no exp, no pow, so the only thing that could differ between two machines is numpy's summation order, and the sha256 of
every case, checked on the CPU, says so.  The blank is the last column, as in the reference.

The kernel gives thread i of 256 the states i * ppt .. (i + 1) * ppt - 1 with ppt = 1, 2, 4, 8, 16, 32, the smallest that covers
the L + 1 states.  The sizes below sit at and around every boundary of that ownership: a lane, a wave (64), the workgroup (256),
and one state past every change of ppt (257, 513, 1025, 2049, 4097).
"""
import hashlib

import numpy as np

STORE_LIMIT = 65536                 # bytes of posterior above which a case is rebuilt from its recipe instead of stored

CASES = {}


def _case(T, S, L, seed, modes=(False, True), seq="random", dtype="float32"):
    return dict(T=T, S=S, L=L, seed=seed, modes=tuple(modes), seq=seq, dtype=dtype)


# the reference's own known answers (test/unit/test_decode.py): inputs in tests/golden/decode.npz, fed as float64
CASES["kat"] = dict(T=10, S=5, L=6, seed=None, modes=(False, True), seq="kat", dtype="float64")
# one, two, three rows; `full` cases keep L <= T / 2, far from the underflow edge
CASES["rows1"] = _case(1, 5, 2, 101, modes=(False,))
CASES["rows1_full"] = _case(1, 5, 0, 102, modes=(True,))
CASES["rows2"] = _case(2, 5, 2, 103, modes=(False,))
CASES["rows2_full"] = _case(2, 5, 1, 104, modes=(True,))
CASES["rows3"] = _case(3, 5, 2, 105, modes=(False,))
CASES["rows3_full"] = _case(3, 5, 1, 106, modes=(True,))
# L + 1 states at and around every ownership boundary, both modes on 2 L + 4 rows
for _n in (1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097):
    CASES["states%d" % _n] = _case(2 * (_n - 1) + 4, 5, _n - 1, 1000 + _n)
# the state count of a 5-mer transducer
CASES["wide_small"] = _case(12, 1025, 5, 201)
CASES["wide_chunk"] = _case(800, 1025, 400, 202)
CASES["rows2000"] = _case(2000, 65, 900, 203)
# one repeated symbol; the symbol next to the blank (S - 2)
CASES["repeat"] = _case(40, 5, 17, 204, seq="repeat")
CASES["sminus2"] = _case(40, 5, 17, 205, seq="sminus2")
CASES["sminus2_wide"] = _case(12, 1025, 6, 206, seq="sminus2")

NAMES = list(CASES)


def make_post(seed, T, S, dtype):
    rs = np.random.RandomState(seed)
    u = rs.uniform(size=(T, S))
    u = u * rs.uniform(size=(T, S))                     # a product of two draws: small values are common, as in a real posterior
    hot = rs.randint(0, S, size=T)
    u[np.arange(T), hot] *= S                           # one boosted column per row
    p = u / np.sum(u, axis=1, keepdims=True)
    return np.ascontiguousarray(p.astype(dtype))


def make_seq(seed, S, L, kind):
    rs = np.random.RandomState(seed + 7919)
    if kind == "repeat":
        return np.full(L, 3 % (S - 1), dtype=np.int64)
    seq = rs.randint(0, S - 1, size=L).astype(np.int64)  # never the blank
    if kind == "sminus2":
        seq[::3] = S - 2
    return seq


def stored(case):
    return case["seed"] is not None and case["T"] * case["S"] * np.dtype(case["dtype"]).itemsize <= STORE_LIMIT


def build(name, kat=None):
    """-> (post, seq) of a named case.  `kat`: the arrays of tests/golden/decode.npz (needed for the case "kat" only)."""
    c = CASES[name]
    if c["seq"] == "kat":
        return np.ascontiguousarray(kat["kat_post"], dtype=np.float64), np.asarray(kat["kat_bases"], dtype=np.int64)
    return make_post(c["seed"], c["T"], c["S"], c["dtype"]), make_seq(c["seed"], c["S"], c["L"], c["seq"])


def digest(post, seq):
    h = hashlib.sha256()
    h.update(str(post.dtype).encode() + repr(post.shape).encode())
    h.update(np.ascontiguousarray(post).tobytes())
    h.update(np.ascontiguousarray(seq, dtype=np.int64).tobytes())
    return h.hexdigest()


def entries():
    """Every scored entry of the fixture: (key, case name, full)."""
    return [("%s/%s" % (n, "full" if f else "free"), n, f) for n in NAMES for f in CASES[n]["modes"]]
