"""Record tests/golden/gru_bar16_bits.npz: what csrc/gru_bar16.hip (slk_gru_bar16_f32, four-chunk plan forced) computes for the cases of
tests/test_gpu_gru_bar16_bits.py (CRC32 of h_out and zr_out, first and last row of h_out).  Run it on the library whose bits are to be
the yardstick -- BEFORE a change of the kernel that must not move a bit -- and never to make a failing test pass.
    python tools/gru_bits_record.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sloika_amd import _lib
    from tests import test_gpu_gru_bar16_bits as t
    _lib.require_gpu()
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    data = {}
    for I, n in t.SHAPES:
        data.update(t.record(I, n))
    np.savez_compressed(out, **data)
    print("%s: %d cases, %d bytes (library %s)" % (out, len(t.SHAPES) * len(t.cases()), os.path.getsize(out), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
