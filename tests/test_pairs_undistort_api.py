"""Undistortion of camera images (mbavo_camera_radtan, mbavo_undistort_map, mbavo_undistort_u8, mbavo_pairs_set_camera,
mbavo_pairs_opts.undistort): what can be held without a GPU.  The entry points exist in the library, the header and the binding;
the options struct keeps its size and `undistort` lies where the header puts it; mbavo_pairs_plan counts the one level-0 map and
rejects other values; and the numpy restatement the GPU tests use as their expectation (tests/pairs_undistort_ref.py) has the
witnesses the three coefficient sets are chosen for: the identity, taps outside the raw image, and none."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_api_support as api
import pairs_undistort_ref as uref
from mba_vo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_camera_radtan_size", "mbavo_undistort_map", "mbavo_undistort_u8", "mbavo_pairs_set_camera"]


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert re.search(r"\bundistort\s*;", header) and re.search(r"\breserved\s*\[\s*3\s*\]", header)
    assert lib.mbavo_abi_version() == 3
    # validated before anything touches a device: no context, no object, no call
    cam = capi.CameraRadTan()
    K = (C.c_double * 4)(100.0, 100.0, 32.0, 24.0)
    assert lib.mbavo_undistort_map(None, C.byref(cam), K, 48, 64, None) == api.E_ARG
    assert lib.mbavo_undistort_u8(None, None, 48, 64, None, 48, 64, None) == api.E_ARG
    assert lib.mbavo_pairs_set_camera(None, C.byref(cam)) == api.E_ARG


def test_structs_have_the_sizes_and_offsets_of_the_header(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    P, Cam = capi.PairsOpts, capi.CameraRadTan
    assert lib.mbavo_pairs_opts_size() == C.sizeof(P) == 272
    assert P.undistort.offset == 256 == P.depth_max.offset + 4 and P.undistort.size == 4
    assert P.reserved.offset == 244 and P.reserved.size == 28  # `reserved` stays the name of the whole tail
    assert lib.mbavo_camera_radtan_size() == C.sizeof(Cam) == 72
    assert (Cam.H.offset, Cam.W.offset, Cam.intrinsics.offset, Cam.dist.offset) == (0, 4, 8, 40)
    o = P()
    assert o.undistort == 0  # a zeroed struct is today's behaviour
    o.undistort = 2
    assert bytes(o)[256:260] == np.array([2], np.int32).tobytes() and list(o.reserved)[3] == 2


def test_plan_counts_one_level_0_map(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for kw in (dict(), dict(B=3, L=2, H=75, W=101, cell=12), dict(B=64, H=480, W=640, fmt=2), dict(B=1, L=1, H=50, W=70)):
        plans = []
        for u in (0, 1, 2):
            o = api.opts(capi, keep=keep, **kw)
            o.undistort = u
            plans.append(api.plan(lib, o))
        assert all(p[0] == 0 for p in plans), plans
        H, W = kw.get("H", 120), kw.get("W", 160)
        extra = plans[1][1] - plans[0][1]
        assert 8 * H * W <= extra < 8 * H * W + 256, (kw, extra)  # ONE map, whatever B is, padded to the arrays' alignment
        assert plans[2][1] == plans[1][1] and plans[0][2] == plans[1][2] == plans[2][2]
    o = api.opts(capi, keep=keep, cell=0)
    o.every_candidate, o.undistort = 1, 1
    z = api.opts(capi, keep=keep, cell=0)
    z.every_candidate = 1
    assert api.plan(lib, o)[0] == 0 and api.plan(lib, o)[1] - api.plan(lib, z)[1] >= 8 * 120 * 160


@pytest.mark.parametrize("value", [3, -1, 256, -2147483648])
def test_plan_rejects_other_values(mbavo, value):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for every in (0, 1):
        o = api.opts(capi, keep=keep)
        o.every_candidate, o.undistort = every, value
        rc, nb, _ = api.plan(lib, o)
        assert rc == api.E_ARG and nb == -7  # (nothing written on an error)
    h = C.c_void_p()  # create validates before it looks at the context
    assert lib.mbavo_pairs_create(None, C.byref(o), C.byref(h)) == api.E_ARG and not h.value


SIZES = [(48, 64), (50, 70), (120, 160), (480, 640)]


@pytest.mark.parametrize("H,W", SIZES)
def test_no_distortion_and_the_same_camera_return_the_image(H, W):
    """Zero coefficients, equal intrinsics, equal sizes: the 1 + 1e-8 of `project` moves every map entry off the grid, and the
    rounding of the remap returns the image byte for byte all the same."""
    K = uref.intrinsics(H, W)
    m = uref.undistort_map(K, uref.DIST_NONE, K, H, W)
    grid = np.stack(np.broadcast_arrays(np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]), 2)
    off = np.abs(m.astype(np.float64) - grid)
    assert m.dtype == np.float32 and m.shape == (H, W, 2) and (off > 0).any() and off.max() < 1e-3
    rng = np.random.default_rng(H)
    for img in (synth.texture_image(H, W, seed=3, octaves=(16, 8, 4)), rng.integers(0, 256, (H, W)).astype(np.uint8),
                np.full((H, W), 255, np.uint8)):
        assert np.array_equal(uref.remap_u8(img, m), img)


@pytest.mark.parametrize("H,W", SIZES[:2])
def test_the_coefficient_sets_have_their_witnesses(H, W):
    """The lens of DIST_OUTSIDE points 1 % .. 10 % of the pixels at a tap outside the raw image, DIST_INSIDE none."""
    K = uref.intrinsics(H, W)
    out = uref.tap_outside(uref.undistort_map(K, uref.DIST_OUTSIDE, K, H, W), H, W)
    print("share of pixels with a tap outside at %d x %d: %.4f" % (H, W, out.mean()))
    assert 0.01 < out.mean() < 0.10
    m = uref.undistort_map(K, uref.DIST_INSIDE, K, H, W)
    assert not uref.tap_outside(m, H, W).any()
    grid_x = np.arange(W, dtype=np.float64)[None, :]
    assert np.abs(m[..., 0] - grid_x).max() > 1.0  # and it is a distortion: corners move by more than a pixel


def test_remap_edges_by_hand():
    """BORDER_CONSTANT 0, the rounding, and the entries that point nowhere, on a 3 x 4 image."""
    src = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 250]], np.uint8)
    Hs, Ws = src.shape
    entries = [(1.0, 1.0), (1.5, 1.0), (1.5, 0.5), (-0.5, 0.0), (Ws - 0.5, 2.0), (3.0, Hs - 1.0), (0.0, -0.5), (-1.0, 0.0), (4.0, 1.0),
               (np.nan, 1.0), (1.0, np.inf), (2.0 ** 31, 1.0), (1.0, -2.0 ** 30), (2.0 ** 30 - 64, 1.0), (0.25, 0.25), (2.5, 1.5)]
    m = np.array(entries, np.float32).reshape(1, -1, 2)
    want = [60, 65, 45, 5, 125, 250, 5, 0, 0, 0, 0, 0, 0, 0, int(0.75 * (0.75 * 10 + 0.25 * 20) + 0.25 * (0.75 * 50 + 0.25 * 60) + 0.5),
            int(0.5 * (0.5 * 70 + 0.5 * 80) + 0.5 * (0.5 * 110 + 0.5 * 250) + 0.5)]
    assert uref.remap_u8(src, m)[0].tolist() == want
    inside, xr, yr = uref.nearest_raw(m, Hs, Ws)
    assert inside[0].tolist() == [True, True, True, True, False, True, True, False, False, False, False, False, False, False, True, True]
    assert (xr[0, 1], yr[0, 2], xr[0, 3], yr[0, 6], xr[0, 15], yr[0, 15]) == (2, 1, 0, 0, 3, 2)  # floor(s + 0.5): halves go up


def test_depth_through_the_map_by_hand():
    raw = np.arange(12, dtype=np.uint16).reshape(3, 4) * 1000
    m = np.array([[(0.4, 0.6), (3.49, 1.5)], [(3.5, 0.0), (np.nan, 0.0)]], np.float32)
    z = uref.depth_through_map(2, raw, m, (1.0, 1.0, 0.0, 0.0), 5000.0)
    assert z.dtype == np.float32 and z.tolist() == [[np.float32(4000 / 5000.0), np.float32(11000 / 5000.0)], [0.0, 0.0]]
    rayd = np.full((3, 4), 2.0, np.float32)
    z = uref.depth_through_map(1, rayd, m, (2.0, 2.0, 0.0, 0.0))
    assert z[0, 0] == 2.0 and z[0, 1] == np.float32(2.0 * (1.0 / np.sqrt(0.25 + 0.0 + 1.0)))  # the ray of (x0, y0) = (1, 0), not of (3, 2)
