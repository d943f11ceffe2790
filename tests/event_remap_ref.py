"""numpy restatement of what `chunkify remap` derives from a remapped path (sloika/batch.py:69-78 on the table batch.remap returns,
sloika/tools/chunkify_with_remap.py:57-58), and the loader of tests/golden/event_remap.npz.  Shared by the host and the GPU tests of
the event remap; nothing here touches a GPU."""
import os
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)
import event_remap_cases as erc  # noqa: E402

_cache = {}


def gold():
    if "gold" not in _cache:
        _cache["gold"] = dict(np.load(os.path.join(GOLD, "event_remap.npz")))
    return _cache["gold"]


def case(name):
    """The regenerated inputs of a case, checked against the digest of what the reference saw; built once."""
    if name not in _cache:
        c = erc.build(name)
        assert erc.digest(c) == str(gold()[name + "_digest"]), "regenerated inputs of %s differ from what the reference saw" % name
        _cache[name] = c
    return _cache[name]


def labels_of_path(path, seq, chunk_len):
    """-> int32 [ml, chunk_len]: seq[path[e]] for the first ml * chunk_len events, 0 where the position repeats the event before
    inside a chunk (a chunk's first event keeps its label)."""
    path, seq = np.asarray(path, dtype=np.int64), np.asarray(seq, dtype=np.int32)
    ml = len(path) // chunk_len
    pos = path[:ml * chunk_len].reshape(ml, chunk_len)
    labels = seq[pos]
    labels[:, 1:][pos[:, 1:] == pos[:, :-1]] = 0
    return labels


def strand_stats(path):
    """-> (nstay, start, end) over ALL events: stays after the first event, the smallest and the largest position."""
    path = np.asarray(path, dtype=np.int64)
    return int((path[1:] == path[:-1]).sum()), int(path.min()), int(path.max())
