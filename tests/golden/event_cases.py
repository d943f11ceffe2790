"""The seeded synthetic event tables behind tests/golden/events.npz, and the float64 yardstick both sides are measured against.
Shared by the generator (make_event_goldens.py) and the tests; nothing here touches the reference or a GPU."""
import numpy as np

#: name -> (events, seed, float dtype of mean / stdv, dtype of 'length' (float: seconds, integer: samples), constant stdv or None)
CASES = {
    "n1": (1, 11, "f8", "f8", None),
    "n2": (2, 12, "f8", "f8", None),
    "n7": (7, 13, "f4", "i8", None),
    "n401": (401, 14, "f8", "f8", 1.5),           # a column whose deviation is exactly 0
    "n2000": (2000, 15, "f8", "f8", None),        # a whole number of chunks of 100 and of 500: no chunk gets the extra event
    "n10750": (10750, 16, "f4", "i8", None),
}
CHUNK_LENS = (100, 500)
NORMALISATIONS = ("none", "per-read", "per-chunk")
SCALED = (1.03125, -2.5)                           # scaled_mean = mean * a + b, scaled_stdv = stdv * a (exact factors)
STUDENTISE_SHAPE = (401, 5)


def columns(name):
    """The stored columns of a case, generated: dict of mean, stdv, length, kmer ('S5'), seq_pos (int32), good_emission (bool)."""
    n, seed, ftype, ltype, const_stdv = CASES[name]
    rs = np.random.RandomState(seed)
    move = rs.rand(n) < 0.7
    seq_pos = np.cumsum(move).astype(np.int32)
    level = rs.normal(size=int(seq_pos.max()) + 1)
    mean = (90.0 + 12.0 * level[seq_pos] + rs.normal(scale=0.8, size=n)).astype(ftype)
    stdv = np.abs(1.5 + 0.4 * rs.normal(size=n)).astype(ftype)
    if const_stdv is not None:
        stdv[:] = const_stdv
    samples = rs.geometric(0.1, size=n) + 2
    length = samples.astype(ltype) if np.dtype(ltype).kind == "i" else (samples / 4000.0).astype(ltype)
    ref = rs.randint(0, 4, size=int(seq_pos.max()) + 5)
    letters = np.frombuffer(b"ACGT", dtype="S1")[ref]
    kmer = np.asarray([b"".join(letters[p:p + 5]) for p in seq_pos], dtype="S5")
    return {"mean": mean, "stdv": stdv, "length": length, "kmer": kmer, "seq_pos": seq_pos, "good_emission": rs.rand(n) > 0.05}


def table(cols):
    """The structured array the reference's functions take, out of stored columns (the 'scaled_' twins are derived)."""
    n = len(cols["mean"])
    ft, lt = cols["mean"].dtype, cols["length"].dtype
    ev = np.zeros(n, dtype=[("mean", ft), ("stdv", ft), ("length", lt), ("scaled_mean", ft), ("scaled_stdv", ft), ("kmer", "S5"),
                            ("seq_pos", "i8"), ("good_emission", "?")])
    for k in ("mean", "stdv", "length", "kmer", "seq_pos", "good_emission"):
        ev[k] = cols[k]
    ev["scaled_mean"] = cols["mean"] * ft.type(SCALED[0]) + ft.type(SCALED[1])
    ev["scaled_stdv"] = cols["stdv"] * ft.type(SCALED[0])
    return ev


def studentise_input():
    return np.random.RandomState(99).normal(loc=3.0, scale=2.0, size=STUDENTISE_SHAPE).astype(np.float32)


def studentise64(x, axis=0):
    """sloika/maths.py:55-58 in float64."""
    x = np.asarray(x, dtype=np.float64)
    m = x.mean(axis=axis, keepdims=True)
    s = x.std(axis=axis, keepdims=True)
    return (x - m) / np.where(s > 0.0, s, 1.0)


def features64(ev, tag, normalise, nanonet):
    """sloika/features.py:16-32 with the moments in float64: the float32 feature values the reference stores into its matrix (the
    delta taken in the table's precision), studentised in float64.  -> float64 [nev, 4]."""
    f = np.zeros((len(ev["length"]), 4), dtype=np.float32)               # (a structured array or a dict of columns)
    f[:, 0], f[:, 1], f[:, 2] = ev[tag + "mean"], ev[tag + "stdv"], ev["length"]
    f[:, 3] = np.fabs(np.ediff1d(ev[tag + "mean"], to_end=0))
    out = studentise64(f) if normalise else f.astype(np.float64)
    if nanonet:
        d = np.ediff1d(ev[tag + "mean"], to_end=0).astype(np.float32).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 3] = d / d.std()
    return out


def chunk_features64(ev, tag, chunk_len):
    """The 'per-chunk' features of sloika/batch.py:37-49 in float64: -> [ml, chunk_len, 4]."""
    ml = len(ev) // chunk_len
    return np.stack([features64(ev[c * chunk_len: min((c + 1) * chunk_len + 1, len(ev))], tag, True, False)[:chunk_len]
                     for c in range(ml)])
