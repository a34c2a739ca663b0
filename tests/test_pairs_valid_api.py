"""The clearance mask (mbavo_pairs_opts.valid_radius, mbavo_undistort_clearance_batch, mbavo_undistort_clearance_bytes): what can
be held without a GPU.  The entries exist in the library, the header and the binding; mbavo_pairs_opts has not grown;
mbavo_pairs_plan counts one clearance pyramid per map and nothing with valid_radius = 0; the two numpy forms of the definitions
(tests/pairs_valid_ref.py) agree; and the cameras the GPU tests use leave them something to drop and something to keep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_api_support as api
import pairs_undistort_ref as uref
import pairs_valid_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_undistort_clearance_batch", "mbavo_undistort_clearance_bytes"]


def _align(v, a=256):
    return (v + a - 1) // a * a


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert re.search(r"\bvalid_radius\s*;", header) and re.search(r"\breserved2\s*\[\s*1\s*\]\s*;", header)
    assert lib.mbavo_abi_version() == 3
    # validated before anything touches a device: no context, no call
    assert lib.mbavo_undistort_clearance_batch(None, 1, None, 50, 70, 60, 80, 3, 1, None) == api.E_ARG


def test_the_options_struct_has_not_grown(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    P = capi.PairsOpts
    assert lib.mbavo_pairs_opts_size() == C.sizeof(P) == 272
    assert P.valid_radius.offset == 264 == P.num_cameras.offset + 4 and P.valid_radius.size == 4
    assert P.reserved.offset == 244 and P.reserved.size == 28  # `reserved` stays the name of the whole tail
    o = P()
    assert o.valid_radius == 0  # a zeroed struct is today's behaviour
    o.valid_radius = 5
    assert bytes(o)[264:268] == np.array([5], np.int32).tobytes() and list(o.reserved)[5] == 5 and list(o.reserved)[6] == 0


@pytest.mark.parametrize("kw", [dict(), dict(B=3, L=3, H=50, W=70, cell=6), dict(B=64, H=480, W=640, fmt=2), dict(B=2, L=8, H=1024, W=1280, cell=40)])
def test_plan_counts_one_clearance_pyramid_per_map(mbavo, kw):
    """valid_radius = 0: the bytes of an object without the field.  r > 0: exactly G' x sum_l aligned(H_l W_l) more, G' =
    max(num_cameras, 1), whatever r is; the capacities do not move."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    B, L, H, W = kw.get("B", 4), kw.get("L", 4), kw.get("H", 120), kw.get("W", 160)
    pyramid = sum(_align((H >> l) * (W >> l)) for l in range(L))
    for u in (1, 2):
        for G in (0, 1, 2, B):
            o = api.opts(capi, keep=keep, **kw)
            o.undistort, o.num_cameras = u, G
            base = api.plan(lib, o)
            assert base[0] == 0
            for r in (1, 2, 64):
                o.valid_radius = r
                rc, nbytes, cells = api.plan(lib, o)
                assert rc == 0 and cells == base[2], (u, G, r)
                assert nbytes - base[1] == max(G, 1) * pyramid, (u, G, r, nbytes - base[1])


def test_plan_rejects_a_bad_radius(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for u, r, ok in ((1, -1, False), (1, 65, False), (2, 1 << 30, False), (1, -(1 << 31), False), (0, 1, False), (0, 64, False),
                     (0, 0, True), (1, 0, True), (1, 1, True), (2, 64, True)):
        o = api.opts(capi, keep=keep)
        o.undistort, o.valid_radius = u, r
        rc, nbytes, _ = api.plan(lib, o)
        assert (rc == 0) == ok and (ok or (rc == api.E_ARG and nbytes == -7)), (u, r, rc)


def test_clearance_bytes_is_the_sum_of_the_levels(mbavo):
    lib = mbavo.load()
    for H, W, L in ((50, 70, 3), (48, 64, 3), (480, 640, 4), (45, 63, 1), (1, 1, 1), (129, 257, 8), (2048, 2048, 8), (128, 128, 8)):
        assert lib.mbavo_undistort_clearance_bytes(H, W, L) == vref.pyramid_bytes(H, W, L), (H, W, L)
    for H, W, L in ((50, 70, 0), (50, 70, 9), (50, 70, -1), (0, 70, 1), (50, 0, 1), (-1, 70, 1), (3, 70, 3), (50, 3, 3), (127, 128, 8),
                    (2048, 2049, 1), (1 << 30, 1 << 30, 1)):
        assert lib.mbavo_undistort_clearance_bytes(H, W, L) < 0, (H, W, L)


@pytest.mark.parametrize("camera", sorted(vref.CAMERAS))
@pytest.mark.parametrize("r", [0, 1, 3])
def test_the_two_numpy_forms_agree(camera, r):
    v0 = vref.valid0(vref.camera_map(vref.CAMERAS[camera]), vref.HS, vref.WS)
    loops, sums = vref.clearance_loops(v0, vref.L, r), vref.clearance(v0, vref.L, r)
    assert [a.shape for a in sums] == vref.level_sizes(vref.H, vref.W, vref.L) == [(50, 70), (25, 35), (12, 17)]
    for a, b in zip(loops, sums):
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
    assert vref.packed(sums).size == vref.pyramid_bytes(vref.H, vref.W, vref.L)


def test_the_two_numpy_forms_agree_on_the_handcrafted_map():
    m, want = vref.handcrafted_map()
    v0 = vref.valid0(m, vref.HS, vref.WS)
    assert len(want) == 19 and sum(want.values()) == 7
    for (r, c), ok in want.items():
        assert bool(v0[r, c]) == ok, (r, c, m[r, c])
    assert int((~v0).sum()) == sum(not ok for ok in want.values())  # every other entry is inside
    for r in (0, 1, 3, 8):
        for a, b in zip(vref.clearance_loops(v0, vref.L, r), vref.clearance(v0, vref.L, r)):
            assert np.array_equal(a, b)
    assert not vref.clearance(v0, vref.L, 8)[2].any()  # r = 8 empties the 12 x 17 level
    # rows 48, 49 and columns 68, 69 belong to no box of the 12 x 17 level: the invalid (49, 69) does not reach it
    inside = v0.copy()
    inside[48:, :], inside[:, 68:] = True, True
    assert not v0[49, 69] and not vref.valid_level(v0, 1)[24, 34] and np.array_equal(vref.valid_level(v0, 2), vref.valid_level(inside, 2))


@pytest.mark.parametrize("camera", sorted(vref.CAMERAS))
def test_level_0_validity_is_no_tap_outside(camera):
    """Where tap_outside is defined as the remap reads it -- a usable entry with a fractional part in both coordinates, so that all
    four taps carry weight -- valid is its complement; an entry on a whole coordinate has a tap of weight 0 that may lie outside."""
    m = vref.camera_map(vref.CAMERAS[camera])
    v0 = vref.valid0(m, vref.HS, vref.WS)
    ok, x0, y0, ax, ay = uref._taps(m)
    four = ok & (ax > 0) & (ay > 0)
    assert four.mean() > 0.9
    assert np.array_equal(v0[four], ~uref.tap_outside(m, vref.HS, vref.WS)[four])
    assert not v0[~ok].any()
    # and on the whole coordinates of the handcrafted map: (Ws - 1, Hs - 1) is valid, its taps of weight 0 lie outside
    hm, _ = vref.handcrafted_map()
    at = np.argwhere((hm[..., 0] == vref.WS - 1) & (hm[..., 1] == vref.HS - 1))
    assert len(at) == 1 and vref.valid0(hm, vref.HS, vref.WS)[tuple(at[0])] and uref.tap_outside(hm, vref.HS, vref.WS)[tuple(at[0])]


@pytest.mark.parametrize("camera", sorted(vref.CAMERAS))
def test_input_condition_of_the_gpu_tests(camera):
    """At 50 x 70 with r = 1 the clearance of level 0 is 1 on at least 25 % and 0 on at least 10 % of the pixels that are more than
    r inside the image: the GPU tests have keypoints to drop and keypoints to keep."""
    r = 1
    v0 = vref.valid0(vref.camera_map(vref.CAMERAS[camera]), vref.HS, vref.WS)
    inner = vref.clearance(v0, vref.L, r)[0][r + 1:vref.H - r - 1, r + 1:vref.W - r - 1]
    print("clear share of the inner pixels, %s: %.4f" % (camera, inner.mean()))
    assert inner.mean() >= 0.25 and 1.0 - inner.mean() >= 0.10
