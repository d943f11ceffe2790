"""The seeded inputs behind tests/golden/remap_long.npz: reads whose references are longer than the 5846 positions the LDS-resident
remap kernel holds, for the tiled one (map_to_sequence_long_body, csrc/transducer.hip; design/remap_long.md).
Shared by the generator (make_remap_long_goldens.py) and both test files; plain numpy, nothing here touches the reference or a GPU.

The generators, the priors and the `needs` machinery are those of remap_slip_cases.py.  Three needs are new here, all about where
tiles of 1024 or 4096 positions end:
    min_jump       a jump of at least that many positions (the slip scan's chain crosses whole tiles)
    lands_after    (modulus, residue): a jump that lands on a position with that residue -- residue 1 is the first position after
                   a multiple of the modulus, residue 0 a tile's own first position
    far_tie        the two best final positions tie exactly and lie more than that many positions apart; the first is taken"""
import numpy as np

import remap_slip_cases as rc
from remap_slip_cases import jumps_of, planted, priors          # noqa: F401  (re-exported for the tests)

NEW_NEEDS = ("min_jump", "lands_after", "far_tie")

CASES = {}


def _case(slip, needs, pri=(False, False), tie_gap=None, **gen):
    return dict(slip=slip, needs=needs, pri=pri, tie_gap=tie_gap, gen=gen)


# A planted jump of n positions has to stay cheaper than its alternatives: with 64 k-mers a matching one turns up every 64
# positions or so, so a read could also hop from match to match for about 64 slips per event.  Hence n is kept below some 25
# positions per event that follows the jump, and `contrast` above n slips (a mismatched event must cost more than the jump).

# one position more than the LDS-resident kernel takes; a jump over more than a 4096-tile
CASES["long_5847"] = _case(5.0, dict(jumps=[4200], min_jump=4096), seed=7001, nev=300, npos=5847, nst=65,
                           jumps=[(50, 4200)], contrast=32768.0)
# no steps at all (end = start + the jumps), so every landing is known: 1005, then 4097 = 4 * 1024 + 1, then 5120 = 5 * 1024
CASES["long_8191"] = _case(5.0, dict(jumps=[1000, 3092, 1023], lands_after=[(1024, 1), (1024, 0)]), seed=7002, nev=300, npos=8191,
                           nst=65, jumps=[(60, 1000), (120, 3092), (200, 1023)], start=5, end=5120, contrast=32768.0)
# the quantised variant with a prior_final that makes two final positions, 1500 apart, share the best score
CASES["long_8192"] = _case(0.0, dict(far_tie=1024), tie_gap=1500, seed=7003, nev=64, npos=8192, nst=65, jumps=[(30, 70)],
                           contrast=0.25, grid=4.0, spread=0.25)
CASES["long_8193"] = _case(5.0, dict(jumps=[65, 5000], min_jump=4096), pri=(True, True), seed=7004, nev=300, npos=8193, nst=65,
                           jumps=[(40, 65), (100, 5000)], start=20, end=8000, contrast=32768.0)
CASES["long_8194"] = _case(2.5, dict(jumps=[2048, 4096], min_jump=4096), seed=7005, nev=300, npos=8194, nst=65,
                           jumps=[(100, 2048), (200, 4096)], contrast=1024.0, neginf=0.2)
CASES["long_11693"] = _case(5.0, dict(jumps=[4200, 6000], min_jump=4096), seed=7006, nev=200, npos=11693, nst=65,
                            jumps=[(50, 4200), (120, 6000)], start=100, contrast=8192.0)
# a read that lives in the last tiles of a long reference
CASES["long_16385"] = _case(5.0, dict(jumps=[4500], min_jump=4096), seed=7007, nev=300, npos=16385,
                            nst=65, jumps=[(60, 4500)], start=11500, contrast=32768.0)
# the one larger case: twice the LDS-resident limit plus one, 2000 events, the k-mer states of a real model
CASES["long_11693_big"] = _case(5.0, dict(jumps=[700, 4200, 64], min_jump=4096), seed=7008, nev=2000, npos=11693, nst=1025,
                                jumps=[(400, 700), (1000, 4200), (1969, 64)], start=91, contrast=2048.0)

NAMES = list(CASES)


def forward_slip0(lt, seq, prior_initial=None):
    """rc.forward_np for slip = 0, where the slip recurrence is a plain running maximum (x - 0 is exact): float32 [npos]."""
    ps = np.zeros(len(seq), dtype=np.float32)
    if prior_initial is not None:
        ps = (ps.astype(np.float64) + prior_initial).astype(np.float32)
    ps = ps + np.fmax(lt[0][seq], lt[0][0])
    for i in range(1, len(lt)):
        row = lt[i]
        stay = ps + row[0]
        step = np.full(len(ps), -np.inf, dtype=np.float32)
        step[1:] = ps[:-1] + row[seq[1:]]
        fs = np.full(len(ps), np.float32(-1e38), dtype=np.float32)
        fs[2:] = np.maximum.accumulate(ps[:-2])
        ps = np.maximum(np.maximum(stay, step), fs + row[seq])
    return ps


def tying_prior_final(lt, seq, gap):
    """rc.tying_prior_final for slip = 0."""
    ps = forward_slip0(lt, seq)
    hi = int(np.argmax(np.where(np.arange(len(ps)) >= gap, ps, -np.inf)))
    lo = hi - gap
    assert np.isfinite(ps[hi]) and np.isfinite(ps[lo])
    pf = np.full(len(ps), -1000.0)
    pf[hi] = 0.0
    pf[lo] = float(ps[hi]) - float(ps[lo])
    return pf


def build(name):
    """-> dict(name, slip, ltrans, seq, pi, pf, planted, needs) of a named case."""
    c = CASES[name]
    lt, seq, path = planted(**c["gen"])
    pi, pf = priors(c["gen"]["seed"] + 5000, len(seq), *c["pri"])
    if c["tie_gap"] is not None:
        assert c["slip"] == 0.0
        pf = tying_prior_final(lt, seq, c["tie_gap"])
    return dict(name=name, slip=c["slip"], ltrans=lt, seq=seq, pi=pi, pf=pf, planted=path, needs=c["needs"])


digest = rc.digest


def unmet(case, path, score):
    """The `needs` of a case that `path` / `score` do NOT show (empty list: the case tests what it is there for)."""
    old = dict(case, needs={k: v for k, v in case["needs"].items() if k not in NEW_NEEDS})
    miss = rc.unmet(old, path, score)
    needs = case["needs"]
    d = jumps_of(path)
    landed = np.asarray(path[1:], dtype=np.int64)
    if "min_jump" in needs and not (d >= needs["min_jump"]).any():
        miss.append("no jump of %d or more" % needs["min_jump"])
    for mod, res in needs.get("lands_after", ()):
        if not ((d >= 2) & (landed % mod == res)).any():
            miss.append("no jump that lands on a position = %d mod %d" % (res, mod))
    if "far_tie" in needs:
        final = (forward_slip0(case["ltrans"], case["seq"], case["pi"]).astype(np.float64) + case["pf"]).astype(np.float32)
        best = np.flatnonzero(final == final.max())
        if not (len(best) == 2 and best[1] - best[0] > needs["far_tie"] and path[-1] == best[0] and score == final.max()):
            miss.append("not exactly two best final positions more than %d apart, the first of them taken" % needs["far_tie"])
    return miss
