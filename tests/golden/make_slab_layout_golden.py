#!/usr/bin/env python3
"""Record tests/golden/slab_layout/<case>.npy for tests/test_gpu_slab_layout.py: the outputs of every case with the library that is
built in the tree.  Run ONCE on a GPU with the library of the commit before the slab layout switch (or with the switch at 0,
-DMBAVO_SLAB_COLMAJOR=0, which is that code); the test then holds every later library to these bits.

    python tests/golden/make_slab_layout_golden.py [out_dir]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402  (first HIP runtime in the process)
import mba_vo_amd  # noqa: E402
import test_gpu_slab_layout as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    mba_vo_amd.load()
    ctx = mba_vo_amd.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        for name in T.CASES:
            sc, r = T.evaluate(mba_vo_amd, ctx, name)
            v = T.pack(r)
            np.save(os.path.join(out, name + ".npy"), v)
            print("%-20s %-36s %-32s %6d doubles  valid %d of %d" % (name, r["kern"], r["kern_c"], v.size, int(r["valid"].sum()), sc.K * sc.P))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
