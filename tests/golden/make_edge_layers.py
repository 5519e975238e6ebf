#!/usr/bin/env python3
"""Write tests/golden/edge_layers.npz: what the first and the last layer of the 2-D network computed BEFORE their kernels were
restructured (tests/test_edge_layers.py::test_same_bits_as_before), one small seeded case each, inputs included.

Made from an emulator build of that earlier commit:

    git worktree add /tmp/before <commit> && (cd /tmp/before && python -m redtail_amd.build emu)
    python tests/golden/make_edge_layers.py /tmp/before/tests/emu/build/librt_stereo_emu.so
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]


def main(emu_lib):
    from redtail_amd import capi
    import test_edge_layers as t
    out = t.golden_cases(t._Host(capi.KernelLib(emu_lib)))
    np.savez_compressed(t.GOLDEN, **out)
    print("wrote %s: %d bytes" % (t.GOLDEN, os.path.getsize(t.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
