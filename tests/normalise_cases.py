"""Inputs for the median/MAD normalisation tests (tests/test_oracle_signal.py on the host, tests/test_gpu_normalise.py on
the device): pure numpy, deterministic, float32 [nchunk, n].

`make(kind, n, nchunk, seed)` gives the everyday and the degenerate signals; `group` and `mirrored` are built for the
selection kernel (csrc/frontend.hip, select_pair): after eight rounds it collects the keys that share the answer's upper
16 bits, finishes on them alone when there are at most 256, and takes the median's upper neighbour from the smallest key
above the answer.  Both families fix HOW MANY samples share those upper bits and WHERE in that group the wanted rank falls;
`upper16_count` counts them from the input alone, so a test can assert that a case still means what its name says.
"""
import numpy as np

KINDS = ("normal", "rounded", "two-valued", "constant", "constant-but-one", "negative", "wide", "signed-zeros", "ascending",
         "descending", "infinite-outliers")
WHERE = ("first", "middle", "last")


def make(kind, n, nchunk, seed):
    """float32 [nchunk, n] of one of KINDS."""
    rs = np.random.RandomState((seed * 7919 + KINDS.index(kind) * 104729 + n) % (2 ** 31))
    x = (rs.normal(size=(nchunk, n)) * 12 + 90).astype(np.float32)
    if kind == "normal":
        pass
    elif kind == "rounded":                                   # integers: duplicates across the median
        x = np.round(x)
    elif kind == "two-valued":
        x = np.where(rs.uniform(size=x.shape) < 0.5, 1.0, 2.0).astype(np.float32)
    elif kind == "constant":                                  # MAD 0: the output is NaN (0/0)
        x[:] = 93.25
    elif kind == "constant-but-one":                          # MAD 0 and one sample that is +inf after the division
        x[:] = 93.25
        if n > 1:
            x[np.arange(nchunk), rs.randint(0, n, size=nchunk)] = 93.5
    elif kind == "negative":                                  # centred on 0: keys of both signs
        x = (x - 90.0).astype(np.float32)
    elif kind == "wide":                                      # twelve octaves of magnitude
        x = (x * np.exp2(rs.randint(-6, 7, size=x.shape))).astype(np.float32)
    elif kind == "signed-zeros":                              # many +0.0 and -0.0 around the median
        x = np.round(rs.normal(size=(nchunk, n)) * 0.6).astype(np.float32)
    elif kind == "ascending":
        x = np.sort(x, axis=1)
    elif kind == "descending":
        x = np.sort(x, axis=1)[:, ::-1]
    elif kind == "infinite-outliers":                         # one +inf and one -inf, away from the middle (only NaN is excluded)
        if n >= 3:                                            # (n = 2 would make the median inf - inf = NaN)
            x[:, n // 5] = np.inf
            x[:, n - 1 - n // 7] = -np.inf
    else:
        raise ValueError(kind)
    assert x.dtype == np.float32 and x.shape == (nchunk, n) and not np.isnan(x).any()
    return x.copy()                                           # (C order with positive strides, whatever the slicing above left)


def _group_values(m):
    assert 1 <= m <= 512
    v = (64.0 + np.arange(m) / 1024.0).astype(np.float32)    # 64 + j/1024: an ulp of 64 is 2^-17, so all share the bits 0x4280....
    assert np.all(v.view(np.uint32) >> 16 == 0x4280) and len(np.unique(v)) == m
    return v


def _shuffled_rows(rs, rows):
    return np.ascontiguousarray(np.stack([r[rs.permutation(len(r))] for r in rows]).astype(np.float32))


def group(n, m, where, nchunk=1, seed=0):
    """`m` distinct samples that share their upper 16 bits, `n - m` filler samples well below ([10, 60]) and well above
    ([70, 120]) them, counted so that rank r = (n - 1) // 2 (the median of an odd count, the lower of the two middle samples of an
    even one) is the group's first, middle or last element.  With 'last' and an even n, rank r + 1 is the smallest upper filler:
    the median's upper neighbour lies just outside the group.  Every chunk has its own filler and its own shuffle."""
    r = (n - 1) // 2
    n_low = {"first": r, "middle": r - m // 2, "last": r - (m - 1)}[where]
    n_up = n - m - n_low
    assert n_low >= 0 and n_up >= 0, (n, m, where)
    rs = np.random.RandomState((seed * 7919 + n * 31 + m * 7 + WHERE.index(where)) % (2 ** 31))
    g = _group_values(m)
    rows = [np.concatenate([rs.uniform(10, 60, size=n_low).astype(np.float32), g,
                            rs.uniform(70, 120, size=n_up).astype(np.float32)]) for _ in range(nchunk)]
    return _shuffled_rows(rs, rows)


def mirrored(n, m, where="middle", nchunk=1, seed=0):
    """Even n; n/2 magnitudes (m of them `group`'s values, the rest filler below and above), each once with either sign: the two
    middle samples are -a and +a, the median is exactly 0, and the MAD selection sees every magnitude twice -- 2m keys share the
    upper bits, and rank r = n/2 - 1 of the deviations falls into the first, a middle or the last pair of them.  With 'last' and
    n a multiple of 4, rank r + 1 is the smallest upper filler."""
    assert n % 2 == 0 and n >= 2
    h, r = n // 2, n // 2 - 1
    n_low = {"first": r // 2, "middle": (r - m + 1) // 2, "last": r // 2 - m + 1}[where]
    n_up = h - m - n_low
    assert n_low >= 0 and n_up >= 0, (n, m, where)
    rs = np.random.RandomState((seed * 7919 + n * 31 + m * 7 + WHERE.index(where) + 1000003) % (2 ** 31))
    g = _group_values(m)
    rows = []
    for _ in range(nchunk):
        mag = np.concatenate([rs.uniform(10, 60, size=n_low).astype(np.float32), g, rs.uniform(70, 120, size=n_up).astype(np.float32)])
        rows.append(np.concatenate([mag, -mag]))
    return _shuffled_rows(rs, rows)


def sort_keys(x):
    """float32 -> uint32 keys that sort like the values (the selection and radix kernels' f2key)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def upper16_count(row):
    """How many samples of one chunk share the upper 16 key bits of its sample of rank (n - 1) // 2: what the selection kernel
    collects after its eighth round."""
    k = np.sort(sort_keys(row))
    return int(np.count_nonzero(k >> 16 == k[(len(k) - 1) // 2] >> 16))


def numpy_med_mad_normalise(x):
    """numpy's own float32 evaluation (sloika/maths.py:4-27, tools/chunkify_raw.py:178-181): -> out, med, mad."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        med = np.median(x, axis=1)
        mad = np.float32(1.4826) * np.median(np.abs(x - med[:, None]), axis=1)
        out = (x - med[:, None]) / mad[:, None]
    assert out.dtype == np.float32 and med.dtype == np.float32 and mad.dtype == np.float32
    return out, med, mad
