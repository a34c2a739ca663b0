"""Shared by the CPU tests of the mbavo_pairs_* argument checks: the options every one of them starts from, the plan call, and
a unified-model camera with xi > 1."""
import ctypes as C

import numpy as np

from mba_vo_amd import synth

E_ARG = -1


def opts(capi, B=4, L=4, H=120, W=160, N=4, k=4, cell=30, fmt=0, keep=None):
    pat = np.ascontiguousarray(synth.PATTERN8, dtype=np.int32)
    if keep is not None:
        keep.append(pat)
    o = capi.PairsOpts()
    o.B, o.L, o.H, o.W, o.spline_deg_k, o.N = B, L, H, W, k, N
    for l in range(8):
        o.S[l], o.P[l] = 8, 8
        o.pattern_xy[l] = pat.ctypes.data_as(capi.c_ip)
        o.border[l] = max(4, 20 >> l)
    for i, v in enumerate((W / 2.0, W / 2.0, W / 2.0, H / 2.0)):
        o.intrinsics[i] = v
    o.huber_a, o.score_threshold, o.cell_H, o.cell_W, o.keyframe_format = 10.0, 4.0, cell, cell, fmt
    return o


def plan(lib, o):
    nbytes, cells = C.c_longlong(-7), (C.c_int * 8)()
    rc = lib.mbavo_pairs_plan(C.byref(o) if o is not None else None, C.byref(nbytes), cells)
    return rc, nbytes.value, list(cells)


XI_ABOVE_1 = dict(model=2, Hs=60, Ws=80, from_intr=(30.0, 30.0, 39.5, 29.5), xi=1.5, dist=(0.0, 0.0, 0.0, 0.0), to_intr=(33.0, 32.5, 31.3, 23.6))
