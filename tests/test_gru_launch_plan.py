"""The launch plan of the whole-layer Gru has one home, layers.gru_launch (chunks per workgroup, two workgroups per CU or one), and
Parallel decides its side-by-side plan without storing it.  tests/golden/gru_launch_plan.json holds what the commit before that change
decided -- its _gru_plan_for, Gru._plan_bits, Gru._forward's and _gru_stack_ok's readings of the bits, Parallel._side_streams and the
library's bar16_auto_plan -- on both sides of every fit threshold of 8 and of 256 CUs, for 1 / 2 / 4 / 8 batches in flight, wide and
narrow layers, with and without `deterministic`, alone and under the side plan a two-direction birnn chooses.  No GPU."""
import copy
import json
import os

import pytest

from sloika_amd import layers

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "gru_launch_plan.json")) as fh:
        doc = json.load(fh)
    assert len(doc["parent"]) == 40 and len(doc["rows"]) == 512
    return doc["rows"]


def _facts(launch):
    return [launch.chunks, launch.share_cu, launch.two_term, launch.stackable]


def test_gru_launch_reproduces_the_recorded_table(table):
    for ncu, B, in_flight, narrow, det, _, side, alone, beside in table:
        where = (ncu, B, in_flight, narrow, det, side)
        assert _facts(layers.gru_launch(B, ncu, narrow, None, in_flight, det)) == alone, where
        side = None if side is None else layers.GruLaunch(*side)
        assert _facts(layers.gru_launch(B, ncu, narrow, side, in_flight, det)) == beside, where


def test_gru_launch_invariants(table):
    seen = set()
    for ncu, B, in_flight, narrow, det, _, side, _, _ in table:
        for s in (None, None if side is None else layers.GruLaunch(*side)):
            launch = layers.gru_launch(B, ncu, narrow, s, in_flight, det)
            seen.add(launch)
            assert launch.chunks in (4, 8, 16)
            assert not (det and launch.chunks == 16)
            assert not launch.share_cu or (narrow and launch.chunks == 4)
            assert launch.two_term == (launch.chunks <= 8)
            assert launch.stackable == (launch.chunks == 4 and not launch.share_cu)
            assert launch.reverse_bits == {4: 1, 8: 2, 16: 3}[launch.chunks] | (4 if launch.share_cu else 0)
    # (the grid reaches every plan there is)
    assert seen == {layers.GruLaunch(4, False), layers.GruLaunch(4, True), layers.GruLaunch(8, False), layers.GruLaunch(16, False)}


def _state(net):
    return [copy.copy(vars(l)) for l in [net] + list(net.layers) + [getattr(l, "layer", l) for l in net.layers]]


@pytest.mark.parametrize("narrow", [False, True])
def test_parallel_decides_its_side_plan_and_stores_nothing(table, narrow):
    """The birnn's choice is the recorded one, and choosing leaves the Parallel, its sub-layers and the Grus inside them as they were (the
    layers of one network are shared by the Basecallers of several host threads: a plan written on them would cross threads)."""
    w = 64 if narrow else 96
    net = layers.birnn(layers.Gru(w, w), layers.Gru(w, w))
    before = _state(net)
    keep = layers._HINTS.in_flight
    try:
        for ncu, B, in_flight, nar, _, together, side, _, _ in table:
            if nar != narrow:
                continue
            layers._HINTS.in_flight = in_flight
            got = net._side_launch(B, ncu)
            assert got == (together, None if side is None else layers.GruLaunch(*side)), (ncu, B, in_flight)
            now = _state(net)
            assert [d.keys() for d in now] == [d.keys() for d in before]
            assert all(a[k] is b[k] for a, b in zip(now, before) for k in a)
    finally:
        layers._HINTS.in_flight = keep
    assert layers._HINTS.gru_side is None


def test_hint_overrides_are_scoped_and_unwind_in_order():
    hints = layers._HINTS
    before = hints.gru_side, hints.in_flight, hints.deterministic
    with hints.override(in_flight=4, deterministic=True):
        assert (hints.gru_side, hints.in_flight, hints.deterministic) == (before[0], 4, True)
        side = layers.GruLaunch(8, False)
        with hints.override(in_flight=2, gru_side=side):
            assert (hints.gru_side, hints.in_flight, hints.deterministic) == (side, 2, True)
            with hints.override(deterministic=False):
                assert (hints.gru_side, hints.in_flight, hints.deterministic) == (side, 2, False)
            assert (hints.gru_side, hints.in_flight, hints.deterministic) == (side, 2, True)
        assert (hints.gru_side, hints.in_flight, hints.deterministic) == (before[0], 4, True)
    assert (hints.gru_side, hints.in_flight, hints.deterministic) == before
    with pytest.raises(RuntimeError):
        with hints.override(in_flight=8, deterministic=True):
            assert (hints.in_flight, hints.deterministic) == (8, True)
            raise RuntimeError("inside the block")
    assert (hints.gru_side, hints.in_flight, hints.deterministic) == before
    # a name that is no hint is refused, and nothing is set on the way
    with pytest.raises(AttributeError):
        with hints.override(in_flight=8, in_fligth=2):
            pass
    assert (hints.gru_side, hints.in_flight, hints.deterministic) == before
