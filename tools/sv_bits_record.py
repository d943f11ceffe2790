"""Record tests/golden/sv_bits.npz: what csrc/softmax_viterbi.hip computes for the cases of tests/test_gpu_sv_bits.py (paths, lengths,
float32 scores, CRC32 of the dumped log-posteriors).  Run it on the library whose bits are to be the yardstick -- BEFORE a change of
the kernel that must not move a bit -- and never to make a failing test pass.     python tools/sv_bits_record.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sloika_amd import _lib
    from tests import test_gpu_sv_bits as t
    _lib.require_gpu()
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    data = {}
    for K in t.KS:
        data.update(t.record(K))
    np.savez_compressed(out, **data)
    print("%s: %d cases, %d bytes (library %s)" % (out, sum(len(t.cases(K)) for K in t.KS), os.path.getsize(out), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
