"""mbavo_pairs_*: what can be held without a GPU.  The entry points exist in the library, the header and the binding; the
options are validated by mbavo_pairs_plan (pure host) exactly as mbavo_pairs_create validates them; the plan's keypoint
capacities are the grid cells of FeatureDetectorBase.cpp:56-64 and its byte count covers the arrays the shapes imply; and the
numpy restatement the GPU tests use as their expectation (tests/pairs_ref.py) is itself pinned to the oracle's detector."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_api_support as api
import pairs_ref
from mba_vo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_create", "mbavo_pairs_destroy", "mbavo_pairs_opts_size", "mbavo_pairs_plan", "mbavo_pairs_prepare",
       "mbavo_pairs_set_motion", "mbavo_pairs_get_knots", "mbavo_pairs_problems", "mbavo_pairs_last_stats"]


def test_new_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_pairs_opts_size() == C.sizeof(capi.PairsOpts)
    assert lib.mbavo_sizeof(10) == -1  # the new struct has its own entry point: no new mbavo_sizeof index
    assert lib.mbavo_abi_version() == 3


def test_plan_rejects_bad_options(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    assert api.plan(lib, api.opts(capi, keep=keep))[0] == 0
    assert api.plan(lib, None)[0] == api.E_ARG
    o = api.opts(capi, keep=keep)
    cells = (C.c_int * 8)()
    nbytes = C.c_longlong(0)
    assert lib.mbavo_pairs_plan(C.byref(o), None, cells) == api.E_ARG
    assert lib.mbavo_pairs_plan(C.byref(o), C.byref(nbytes), None) == api.E_ARG
    bad = [dict(L=0), dict(L=9), dict(N=17), dict(H=60, L=4), dict(W=63, L=4), dict(cell=0), dict(fmt=3), dict(fmt=-1), dict(B=0),
           dict(k=3), dict(N=3, k=4), dict(H=2048, W=2056)]  # (the last: more than 2^22 pixels)
    for kw in bad:
        rc, nb, _ = api.plan(lib, api.opts(capi, keep=keep, **kw))
        assert rc == api.E_ARG and nb == -7, kw  # (nothing written on an error)
    o = api.opts(capi, keep=keep)
    o.cell_W = 0
    assert api.plan(lib, o)[0] == api.E_ARG
    o = api.opts(capi, keep=keep)
    o.pattern_xy[2] = None  # a level < L without a pattern
    assert api.plan(lib, o)[0] == api.E_ARG
    o = api.opts(capi, keep=keep)
    o.S[1] = 0
    assert api.plan(lib, o)[0] == api.E_ARG
    o = api.opts(capi, keep=keep)
    o.border[0] = -1
    assert api.plan(lib, o)[0] == api.E_ARG
    o = api.opts(capi, L=4, cell=2, keep=keep)  # int(2 / 1.414^3) = 0: the reference divides by zero there
    assert api.plan(lib, o)[0] == api.E_ARG
    # (H >> (L-1)) == 8 is the smallest admitted
    assert api.plan(lib, api.opts(capi, H=64, W=64, L=4, cell=8, keep=keep))[0] == 0


@pytest.mark.parametrize("B,L,H,W,cell,fmt", [(1, 1, 120, 160, 30, 0), (3, 3, 150, 202, 12, 1), (16, 4, 480, 640, 30, 2), (512, 4, 480, 640, 30, 0),
                                              (512, 4, 480, 640, 30, 2), (2, 8, 1024, 1280, 40, 0)])
def test_plan_of_valid_options(mbavo, B, L, H, W, cell, fmt):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    rc, nbytes, cells = api.plan(lib, api.opts(capi, B=B, L=L, H=H, W=W, cell=cell, fmt=fmt, keep=keep))
    assert rc == 0
    want = pairs_ref.cells_per_level(H, W, L, cell, cell)
    assert cells == want + [0] * (8 - L)
    px = sum((H >> l) * (W >> l) for l in range(L))
    floor = 2 * B * px + B * px * (8 if fmt == 0 else 4) + B * sum(want) * 24 + B * L * 4  # images, gradients, keypoints, counts
    assert nbytes >= floor
    assert nbytes <= 1.05 * floor + (1 << 20)  # padding and the small tables only: the figure is the arrays' size


def test_plan_memory_figures(mbavo):
    """512 pairs of 640 x 480 x 4 levels: ~2.2 GB with float gradients, about half packed."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    f = api.plan(lib, api.opts(capi, B=512, H=480, W=640, fmt=0, keep=keep))[1]
    p = api.plan(lib, api.opts(capi, B=512, H=480, W=640, fmt=2, keep=keep))[1]
    assert 2.0e9 < f < 2.4e9 and 0.5 * f < p < 0.65 * f


def test_create_with_null_arguments(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    o = api.opts(capi, keep=keep)
    h = C.c_void_p()
    assert lib.mbavo_pairs_create(None, C.byref(o), C.byref(h)) == api.E_ARG
    assert lib.mbavo_pairs_create(None, None, C.byref(h)) == api.E_ARG
    assert lib.mbavo_pairs_create(None, C.byref(o), None) == api.E_ARG
    assert not h.value
    for fn in ("mbavo_pairs_destroy",):
        assert getattr(lib, fn)(None) == api.E_ARG
    out = (C.c_longlong * 4)()
    assert lib.mbavo_pairs_last_stats(None, out) == api.E_ARG
    assert lib.mbavo_pairs_prepare(None, None, None, None, None) == api.E_ARG
    assert lib.mbavo_pairs_get_knots(None, None, None) == api.E_ARG
    assert lib.mbavo_pairs_problems(None, None, None) == api.E_ARG
    assert lib.mbavo_pairs_set_motion(None, None, None, None, 0.5, None, None) == api.E_ARG


def test_restatement_matches_the_oracle_detector(orc):
    """tests/pairs_ref.py (grid geometry, selection, depth test, border, order) against the oracle's detector on small images:
    textured with a flat region, odd level sizes, a depth map with holes, a threshold that leaves two equal maxima in a cell,
    a constant image."""
    rng = np.random.default_rng(3)
    dropped_depth = dropped_border = 0
    for (H0, W0, levels, seed) in ((96, 128, 3, 5), (150, 202, 3, 6), (75, 101, 2, 7)):
        img = synth.texture_image(H0, W0, seed=seed, octaves=(32, 16, 8, 4))
        img[10:30, 40:90] = 128
        depth = rng.uniform(0.0, 3.0, (H0, W0)).astype(np.float32)
        depth[depth < 0.4] = 0.0
        for lv, im in enumerate(synth.pyramid(img, levels)):
            H, W = im.shape
            assert (H, W) == (H0 >> lv, W0 >> lv)
            for cell, thr, border in ((12, 3.0, 0), (30, 0.5, max(4, 20 >> lv)), (7, 8.0, 3)):
                (wxy, wz), mag = pairs_ref.oracle_keypoints(orc, im, lv, H0, W0, cell, thr, depth, border)
                assert np.array_equal(pairs_ref.gradient_magnitude(im), mag)
                gxy, gz = pairs_ref.keypoints(im, lv, H0, W0, cell, cell, thr, depth, border)
                assert len(gz) > 0 and np.array_equal(gxy, wxy) and np.array_equal(gz, wz), (H0, lv, cell)
                full = sum(p is not None for p in pairs_ref.picks(mag, lv, H0, W0, cell, cell, thr))
                nob = len(pairs_ref.keypoints(im, lv, H0, W0, cell, cell, thr, depth, 0)[1])
                dropped_depth += full - nob
                dropped_border += nob - len(gz)
    assert dropped_depth > 0 and dropped_border > 0
    # two equal maxima in one cell: the lower row-major index wins
    im = np.full((40, 40), 100, np.uint8)
    im[5, 6] = im[7, 3] = 160  # |gradient| 30 at their four neighbours each; first in row-major order: (6, 4)
    depth = np.ones((40, 40), np.float32)
    (wxy, wz), mag = pairs_ref.oracle_keypoints(orc, im, 0, 40, 40, 20, 1.0, depth, 0)
    assert (mag == mag.max()).sum() >= 8
    gxy, gz = pairs_ref.keypoints(im, 0, 40, 40, 20, 20, 1.0, depth, 0)
    assert np.array_equal(gxy, wxy) and np.array_equal(gz, wz) and gxy.tolist() == [[6.0, 4.0]]
    # constant image: nothing
    im = np.full((40, 56), 77, np.uint8)
    (wxy, wz), _ = pairs_ref.oracle_keypoints(orc, im, 0, 40, 56, 10, 0.5, np.ones((40, 56), np.float32), 0)
    gxy, gz = pairs_ref.keypoints(im, 0, 40, 56, 10, 10, 0.5, np.ones((40, 56), np.float32), 0)
    assert len(wz) == 0 and len(gz) == 0
