"""The workspace arithmetic of the checkpointed lattice marginals (slk_viterbi_marginals_ckpt_workspace_bytes, host only) and the host
side of `checkpoint=` and of the bucketing by footprint: no device needed (design/lattice_marginals.md 8)."""
import pytest


@pytest.fixture(scope="module")
def L():
    from sloika_amd import build, _lib
    build.build()
    return _lib.lib()


def test_a_fifth_of_the_stored_rows_at_a_whole_read(L):
    stored = L.slk_viterbi_marginals_workspace_bytes(20000, 1, 4, 5)
    ckpt = L.slk_viterbi_marginals_ckpt_workspace_bytes(20000, 1, 4, 5, 8)
    assert 0 < 5 * ckpt <= stored
    # 2500 checkpoints of 13 N bytes, 20 bytes per row, rounded up to 256
    assert ckpt == 256 * ((2500 * 13 * 1024 + 20000 * 20 + 255) // 256)
    assert L.slk_viterbi_marginals_ckpt_workspace_bytes(20001, 1, 4, 5, 8) == 256 * ((2501 * 13 * 1024 + 20001 * 20 + 255) // 256)


def test_monotone_in_rows_and_chunks(L):
    for nbase, klen in ((4, 3), (5, 3), (4, 5)):
        for every in (0, 1, 3, 8):
            last = 0
            for T in (1, 2, 3, 8, 9, 17, 800, 801, 20000):
                now = L.slk_viterbi_marginals_ckpt_workspace_bytes(T, 3, nbase, klen, every)
                assert now >= last > 0 or (last == 0 and now > 0), (nbase, klen, every, T)
                last = now
            last = 0
            for B in (1, 2, 5, 64, 256):
                now = L.slk_viterbi_marginals_ckpt_workspace_bytes(800, B, nbase, klen, every)
                assert now > last, (nbase, klen, every, B)
                last = now
    # more rows per checkpoint, less workspace
    sizes = [L.slk_viterbi_marginals_ckpt_workspace_bytes(20000, 4, 4, 5, k) for k in (1, 2, 4, 8, 15)]
    assert sizes == sorted(sizes, reverse=True) and len(set(sizes)) == 5


def test_zero_for_illegal_dimensions(L):
    for shape in ((10, 2, 4, 2), (10, 2, 4, 6), (10, 2, 5, 5), (10, 2, 3, 3), (10, 2, 2, 3), (0, 2, 4, 3), (10, 0, 4, 3)):
        assert L.slk_viterbi_marginals_ckpt_workspace_bytes(*(shape + (4,))) == 0, shape
        assert L.slk_viterbi_marginals_ckpt_workspace_bytes(*(shape + (0,))) == 0, shape
    assert L.slk_viterbi_marginals_ckpt_workspace_bytes(10, 2, 4, 3, -1) == 0


def test_the_default_rows_per_checkpoint(L):
    """every = 0 is the launcher's choice; decode.marginals_default_rows restates it."""
    from sloika_amd import decode
    want = {(4, 3): 64, (5, 3): 32, (4, 4): 16, (5, 4): 6, (4, 5): 4}
    for (nbase, klen), k in want.items():
        assert decode.marginals_default_rows(nbase, klen) == k
        for T in (1, 100, 1001):
            assert (L.slk_viterbi_marginals_ckpt_workspace_bytes(T, 2, nbase, klen, 0)
                    == L.slk_viterbi_marginals_ckpt_workspace_bytes(T, 2, nbase, klen, k)), (nbase, klen, T)
    assert decode.marginals_workspace_bytes(800, 3, 4, 5) == L.slk_viterbi_marginals_workspace_bytes(800, 3, 4, 5)
    assert decode.marginals_workspace_bytes(800, 3, 4, 5, True) == L.slk_viterbi_marginals_ckpt_workspace_bytes(800, 3, 4, 5, 0)
    assert decode.marginals_workspace_bytes(800, 3, 4, 5, 4) == L.slk_viterbi_marginals_ckpt_workspace_bytes(800, 3, 4, 5, 4)
    assert decode.marginals_rows_per_checkpoint(None) is None and decode.marginals_rows_per_checkpoint(True) == 0
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError):
            decode.marginals_rows_per_checkpoint(bad)


def test_length_buckets_close_on_a_footprint():
    from sloika_amd.pipeline import Basecaller
    nsamp = [1000, 990, 980, 970, 500, 495, 490]
    assert Basecaller.length_buckets(nsamp, 256, 0.08) == [[0, 1, 2, 3], [4, 5, 6]]
    assert Basecaller.length_buckets(nsamp, 256, 0.08, None) == [[0, 1, 2, 3], [4, 5, 6]]
    by_bytes = Basecaller.length_buckets(nsamp, 256, 0.08, (lambda longest, reads: longest * reads, 2000))
    assert by_bytes == [[0, 1], [2, 3], [4, 5, 6]]
    with pytest.raises(ValueError, match="read b"):
        Basecaller._check_footprints([10, 30], ["a", "b"], (lambda longest, reads: longest * reads, 20))
