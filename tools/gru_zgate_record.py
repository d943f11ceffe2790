"""Record tests/golden/gru_zgate_bits.npz: what the four-chunk Gru kernel (csrc/gru_bar16_body.h: unpacked, packed, stacked, SAVE)
computes for the cases of tests/test_gpu_gru_zgate_bits.py (CRC32 of every output, first and last row as float32 bit patterns).  Run it
on the library whose bits are to be the yardstick -- BEFORE a change of the kernel that must not move a bit -- and never to make a
failing test pass.
    python tools/gru_zgate_record.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sloika_amd import _lib
    from tests import test_gpu_gru_zgate_bits as t
    _lib.require_gpu()
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    data, ncase = {}, 0
    for mode, I, n in t.RUNS:
        data.update(t.record(mode, I, n))
        ncase += len(t.cases(mode))
    np.savez_compressed(out, **data)
    print("%s: %d cases, %d bytes (library %s)" % (out, ncase, os.path.getsize(out), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
