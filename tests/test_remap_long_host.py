"""The host side of the long-reference remap (design/remap_long.md): the workspace size, the cut of a batch into launches by
workspace_limit, the mirrored default tile and the keyword on every function of the chain.  No GPU needed."""
import inspect
import os
import re

import pytest

from tests.conftest import ROOT



@pytest.fixture(scope="module")
def L():
    from sloika_amd import build, _lib
    build.build()
    return _lib.lib()


def test_workspace_is_the_traceback_and_two_score_rows(L):
    f = L.slk_map_to_sequence_long_workspace_bytes
    for tile in (0, 64, 128, 4096, 6784):
        assert f(10, 100, tile) == 4 * 10 * 100 + 2 * 4 * (100 + 16)
        assert f(23000, 6600, tile) == 4 * 23000 * 6600 + 8 * 6616
        assert f(100000, 30000, tile) == 4 * 100000 * 30000 + 8 * 30016          # past 2^32 bytes
    assert f(1, 3, 0) == 12 + 8 * 19
    for tile in (-64, 1, 32, 63, 96, 100, 6784 + 64, 1 << 30):                   # 6784: the longest tile 160 KB of LDS hold
        assert f(10, 100, tile) == 0, tile
    assert f(0, 100, 0) == 0 and f(10, 0, 0) == 0


def test_default_tile_mirrors_the_kernel_source():
    from sloika_amd import transducer
    with open(os.path.join(ROOT, "sloika_amd", "csrc", "transducer.hip")) as fh:
        m = re.search(r"#define MAP_LONG_TILE_DEFAULT (\d+)", fh.read())
    assert m and int(m.group(1)) == transducer.DEFAULT_TILE
    assert transducer.DEFAULT_TILE % 64 == 0 and 64 <= transducer.DEFAULT_TILE <= 6784


def test_workspace_runs_are_consecutive_and_within_the_limit():
    from sloika_amd import transducer
    from sloika_amd.transducer import workspace_runs
    assert transducer.MAX_POSITIONS == 5846 and transducer.WORKSPACE_LIMIT == 8 << 30
    assert workspace_runs([5, 5, 5, 20, 1, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]
    assert workspace_runs([5, 5], 10) == [(0, 2)]                   # the limit itself is allowed
    assert workspace_runs([11], 10) == [(0, 1)]                     # a read above the limit runs alone
    assert workspace_runs([11, 12, 13], 1) == [(0, 1), (1, 2), (2, 3)]
    assert workspace_runs([3, 3, 3, 3], 1 << 40) == [(0, 4)]
    sizes = [(7 * i) % 13 + 1 for i in range(50)]
    for limit in (1, 5, 13, 20, 100):
        runs = workspace_runs(sizes, limit)
        assert runs[0][0] == 0 and runs[-1][1] == 50 and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert all(hi > lo and (sum(sizes[lo:hi]) <= limit or hi - lo == 1) for lo, hi in runs)
        # greedy: the read after a run would not have fitted into it
        assert all(sum(sizes[lo:hi + 1]) > limit for lo, hi in runs[:-1])


def test_the_keyword_is_on_every_function_of_the_chain_and_off_by_default():
    from sloika_amd import batch, chunkify_raw, transducer
    for f in (transducer.map_to_sequence, transducer.map_to_sequence_batch, transducer.map_to_sequence_packed, batch.remap,
              batch.remap_many, batch.chunk_remap_worker, batch.chunk_remap_many, chunkify_raw.raw_remap, chunkify_raw.raw_remap_many,
              chunkify_raw.raw_chunk_remap_worker):
        assert inspect.signature(f).parameters["long_reference"].default is False, f.__name__
    for f in (transducer.map_to_sequence_batch, transducer.map_to_sequence_packed, batch.remap_many, batch.chunk_remap_many,
              chunkify_raw.raw_remap_many):
        assert "workspace_limit" in inspect.signature(f).parameters, f.__name__
