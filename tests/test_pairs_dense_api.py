"""mbavo_pairs_opts.every_candidate: what can be held without a GPU.  The numpy restatement the GPU tests use as their expectation
(tests/pairs_dense_ref.py) is pinned to the oracle's detector with no grid (orc_detect_semidense, cell 0, then orc_keypoint_depths
and the border filter); mbavo_pairs_plan accepts the mode with cell_H = cell_W = 0, reports H_l * W_l keypoints per level and a
byte count that is the arrays' size, and rejects every other value of the field."""
import ctypes as C

import numpy as np
import pytest

import pairs_api_support as api
import pairs_dense_ref as dref
import pairs_ref
from mba_vo_amd import synth


def test_restatement_matches_the_oracle_detector(orc):
    """The image families of test_pairs_api.test_restatement_matches_the_oracle_detector: textured with a flat region, odd level
    sizes, a depth map with holes; three thresholds and borders.  The depth test and the border test each drop a candidate."""
    rng = np.random.default_rng(3)
    dropped_depth = dropped_border = 0
    for (H0, W0, levels, seed) in ((96, 128, 3, 5), (150, 202, 3, 6), (75, 101, 2, 7)):
        img = synth.texture_image(H0, W0, seed=seed, octaves=(32, 16, 8, 4))
        img[10:30, 40:90] = 128
        depth = rng.uniform(0.0, 3.0, (H0, W0)).astype(np.float32)
        depth[depth < 0.4] = 0.0
        for lv, im in enumerate(synth.pyramid(img, levels)):
            H, W = im.shape
            for thr, border in ((3.0, 0), (0.5, max(4, 20 >> lv)), (8.0, 3)):
                (wxy, wz), mag = pairs_ref.oracle_keypoints(orc, im, lv, H0, W0, 0, thr, depth, border)
                gxy, gz = dref.keypoints(im, lv, thr, depth, border)
                assert len(gz) > 0 and np.array_equal(gxy, wxy) and np.array_equal(gz, wz), (H0, lv, thr)
                full = int((mag > np.float32(thr)).sum())
                nob = len(dref.keypoints(im, lv, thr, depth, 0)[1])
                assert full <= H * W and len(gz) <= nob <= full
                dropped_depth += full - nob
                dropped_border += nob - len(gz)
                # row-major order, no pixel twice
                flat = gxy[:, 1] * W + gxy[:, 0]
                assert np.all(np.diff(flat) > 0)
    assert dropped_depth > 0 and dropped_border > 0
    # constant image: nothing
    im = np.full((40, 56), 77, np.uint8)
    (wxy, wz), _ = pairs_ref.oracle_keypoints(orc, im, 0, 40, 56, 0, 0.5, np.ones((40, 56), np.float32), 0)
    gxy, gz = dref.keypoints(im, 0, 0.5, np.ones((40, 56), np.float32), 0)
    assert len(wz) == 0 and len(gz) == 0 and gxy.shape == (0, 2)


@pytest.mark.parametrize("H,W", [(40, 56), (33, 31), (64, 300)])
def test_ramp_image_has_every_interior_pixel(orc, H, W):
    """(c + r) % 251, depth 1 everywhere, border 0: K = (H - 2)(W - 2), the largest a level can have, in row-major order."""
    im = dref.ramp(H, W)
    depth = np.ones((H, W), np.float32)
    (wxy, wz), _ = pairs_ref.oracle_keypoints(orc, im, 0, H, W, 0, 1.0, depth, 0)
    gxy, gz = dref.keypoints(im, 0, 1.0, depth, 0)
    assert len(gz) == (H - 2) * (W - 2)
    assert np.array_equal(gxy, wxy) and np.array_equal(gz, wz) and np.all(gz == 1.0)
    ys, xs = np.mgrid[1:H - 1, 1:W - 1]
    assert np.array_equal(gxy, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64))


def _dense(capi, keep, every=1, cell=0, **kw):
    o = api.opts(capi, keep=keep, cell=cell, **kw)
    o.every_candidate = every
    return o


def test_binding_mirrors_the_option(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    assert lib.mbavo_pairs_opts_size() == C.sizeof(capi.PairsOpts)
    assert capi.PairsOpts.every_candidate.offset == capi.PairsOpts.keyframe_format.offset + 4
    assert capi.PairsOpts.reserved.size == 7 * 4


@pytest.mark.parametrize("B,L,H,W,fmt", [(1, 1, 120, 160, 0), (3, 3, 50, 70, 1), (16, 4, 480, 640, 2), (64, 4, 480, 640, 0), (2, 2, 2048, 2048, 0)])
def test_plan_of_the_mode(mbavo, B, L, H, W, fmt):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    rc, nbytes, cells = api.plan(lib, _dense(capi, keep, B=B, L=L, H=H, W=W, fmt=fmt))
    assert rc == 0
    want = [(H >> l) * (W >> l) for l in range(L)]
    assert want == dref.capacities(H, W, L) and cells == want + [0] * (8 - L)
    px = sum(want)
    floor = 2 * B * px + B * px * (8 if fmt == 0 else 4) + B * px * 24 + B * L * 4  # images, gradients, keypoints, counts
    assert nbytes >= floor
    assert nbytes <= 1.05 * floor + (1 << 20)  # padding and the small tables only: no pick array
    # cell_H, cell_W are not read
    assert api.plan(lib, _dense(capi, keep, B=B, L=L, H=H, W=W, fmt=fmt, cell=30))[1:] == (nbytes, cells)


def test_plan_memory_figure(mbavo):
    """9.8 MB of keypoints per 640 x 480 x 4 pair: ~0.63 GB at B = 64."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    dense = api.plan(lib, _dense(capi, keep, B=64, H=480, W=640))[1]
    grid = api.plan(lib, api.opts(capi, keep=keep, B=64, H=480, W=640))[1]
    assert 0.60e9 < dense - grid < 0.66e9


def test_plan_rejects_other_values(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for every in (2, -1):
        for cell in (0, 30):
            rc, nb, _ = api.plan(lib, _dense(capi, keep, every=every, cell=cell))
            assert rc == api.E_ARG and nb == -7, (every, cell)
    assert api.plan(lib, _dense(capi, keep, every=0, cell=0))[0] == api.E_ARG  # grid selection needs its cells, as before
    assert api.plan(lib, _dense(capi, keep, every=0, cell=30))[0] == 0
    # what the mode does not change: the other options are validated as ever
    for kw in (dict(L=0), dict(fmt=3), dict(H=60, L=4), dict(B=0), dict(H=2048, W=2056)):
        assert api.plan(lib, _dense(capi, keep, **kw))[0] == api.E_ARG, kw
    o = _dense(capi, keep)
    o.border[1] = -1
    assert api.plan(lib, o)[0] == api.E_ARG
