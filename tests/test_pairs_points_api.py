"""Keypoints and depths from the caller (mbavo_pairs_prepare_points, _update_points, _track_frame_points): what can be held
without a GPU.  The three entries exist in the library, the header and the binding, mbavo_pairs_opts has not grown, the ABI
revision has not moved, and the entries return MBAVO_E_ARG before they touch a device; the numpy restatement of the header's rule
(tests/pairs_points_ref.py) gives, on hand-made points, what the header says by hand, and its two forms agree on random lists.

One reading is fixed here: the header keeps a point whose depth is finite and not below 1e-2, so z = 1e300 is KEPT (unchanged),
while 1e300 in a coordinate fails the 2^30 test and is dropped, as NaN and +-inf are in every field."""
import ctypes as C
import os
import re

import numpy as np

import pairs_mask_ref as mref
import pairs_points_ref as pref
import pairs_valid_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_prepare_points", "mbavo_pairs_update_points", "mbavo_pairs_track_frame_points"]
E_ARG = -1
H, W, BORDERS = 72, 96, (3, 2, 1)


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_abi_version() == 3
    assert lib.mbavo_pairs_opts_size() == C.sizeof(capi.PairsOpts) == 272  # the feature is a set of calls, not an option


def test_the_entries_return_e_arg_before_they_touch_a_device(mbavo):
    lib = mbavo.load()
    assert lib.mbavo_pairs_prepare_points(None, None, None, None, None, None, None) == E_ARG
    assert lib.mbavo_pairs_update_points(None, None, 0, None, None, None, None, None, None) == E_ARG
    assert lib.mbavo_pairs_track_frame_points(None, None, 0, None, None, None, None, None, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None, None) == E_ARG


def test_the_wrapper_has_the_three_calls(mbavo):
    from mba_vo_amd import workloads
    for name in ("prepare_points", "update_points", "track_frame_points"):
        assert callable(getattr(workloads.PairBatch, name))


# ---- the restatement on hand-made points
def _at(x0, y0, z, l, m=None, clear_l=None):
    return pref.kept_at(x0, y0, z, l, H >> l, W >> l, BORDERS[l] if m is None else m, clear_l)


def test_rounding_at_the_image_edges():
    assert _at(-0.5, 36.0, 1.5, 0, m=0) == (0, 36)                       # floor(-0.5 + 0.5) = 0: pixel 0, kept with border 0
    assert _at(-0.5, 36.0, 1.5, 0) is None                               # ... and inside the band with border 3
    assert _at(np.nextafter(-0.5, -1.0), 36.0, 1.5, 0, m=0) is None      # pixel -1
    assert _at(W - 0.5, 36.0, 1.5, 0, m=0) is None                       # pixel W
    assert _at(np.nextafter(W - 0.5, 0.0), 36.0, 1.5, 0, m=0) == (W - 1, 36)
    assert _at(48.0, H - 0.5, 1.5, 0, m=0) is None and _at(48.0, -0.5, 1.5, 0, m=0) == (48, 0)
    assert _at(2.5, 3.5, 1.5, 0, m=0) == (3, 4)                          # halves round up, as (int)(x + 0.5) does for x >= 0
    assert _at(-0.5, 36.0, 1.5, 2, m=0) == (0, 9) and _at(-2.0, 36.0, 1.5, 2, m=0) == (0, 9) and _at(-2.5, 36.0, 1.5, 2, m=0) is None


def test_the_depth_test():
    assert _at(48.0, 36.0, 0.01, 0) == (48, 36) and _at(48.0, 36.0, 0.0099, 0) is None
    assert _at(48.0, 36.0, np.nextafter(0.01, 0.0), 0) is None
    assert _at(48.0, 36.0, 0.0, 0) is None and _at(48.0, 36.0, -3.0, 0) is None
    assert _at(48.0, 36.0, 1e300, 0) == (48, 36)                         # finite and not below 1e-2


def test_no_number_and_too_large():
    nan, inf = float("nan"), float("inf")
    for l in range(3):
        for bad in (nan, inf, -inf, 1e300, -1e300, 2.0 ** 30 * (1 << l), -(2.0 ** 30) * (1 << l)):
            assert _at(bad, 36.0, 1.5, l) is None and _at(48.0, bad, 1.5, l) is None, (l, bad)
        for bad in (nan, inf, -inf):
            assert _at(48.0, 36.0, bad, l) is None, (l, bad)
    assert _at(np.nextafter(2.0 ** 30, 0.0), 36.0, 1.5, 0, m=0) is None  # usable, and far outside the image


def test_a_point_in_level_0s_band_that_level_2_keeps():
    x0, y0 = 2.0, 36.0
    assert _at(x0, y0, 1.5, 0) is None                                   # x = 2 < 3
    assert _at(x0, y0, 1.5, 1) is None                                   # x = 1 < 2
    assert _at(x0, y0, 1.5, 2) == (1, 9)                                 # floor(0.5 + 0.5) = 1 >= 1
    kxy, kz = zip(*[pref.level_keypoints([[x0, y0]], [1.5], l, H >> l, W >> l, BORDERS[l]) for l in range(3)])
    assert [len(z) for z in kz] == [0, 0, 1] and kxy[2].tolist() == [[1.0, 9.0]]


def test_two_points_on_one_level_2_pixel_are_both_kept_in_order():
    xy, z = [[40.0, 20.0], [60.0, 30.0], [41.0, 21.0], [39.0, 19.0]], [2.0, 3.0, 1.0, 4.0]
    k0, z0 = pref.level_keypoints(xy, z, 0, H, W, BORDERS[0])
    k2, z2 = pref.level_keypoints(xy, z, 2, H >> 2, W >> 2, BORDERS[2])
    assert k0.tolist() == xy and z0.tolist() == z
    assert k2.tolist() == [[10.0, 5.0], [15.0, 8.0], [10.0, 5.0], [10.0, 5.0]] and z2.tolist() == z  # nothing is de-duplicated
    assert k2.dtype == np.float64 and z2.dtype == np.float64


def test_the_edge_list_says_what_the_definition_says():
    for x0, y0, z, want in pref.edge_points(H, W, BORDERS):
        for l, kept in want.items():
            assert (_at(x0, y0, z, l) is not None) == kept, (x0, y0, z, l)
    for x0, y0, z, want in pref.edge_points(H, W, (0, 0, 0)):
        for l, kept in want.items():
            assert (_at(x0, y0, z, l, m=0) is not None) == kept, (x0, y0, z, l)


def test_the_two_forms_agree_on_random_lists_with_and_without_a_clearance_pyramid():
    rng = np.random.default_rng(3)
    h, w, L = vref.H, vref.W, vref.L
    clear = mref.clearance(vref.camera_map(vref.CAMERAS["radtan"]), mref.bonnet_undistorted(), L, 1)
    n = 400
    xy = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1)
    xy[::7] = np.floor(xy[::7]) + 0.5  # halves
    xy[::11] = np.floor(xy[::11])
    z = rng.uniform(0.0, 0.03, n)
    z[::5] = rng.uniform(0.5, 3.0, len(z[::5]))
    for k, (x0, y0, zz, _) in enumerate(pref.edge_points(72, 96, (0, 0, 0))):
        xy[3 * k], z[3 * k] = (x0, y0), zz
    for pyramid in (None, clear):
        for l in range(L):
            kxy, kz = pref.level_keypoints(xy, z, l, h >> l, w >> l, BORDERS[l], None if pyramid is None else pyramid[l])
            want = [(pref.kept_at(xy[i, 0], xy[i, 1], z[i], l, h >> l, w >> l, BORDERS[l], None if pyramid is None else pyramid[l]), z[i]) for i in range(n)]
            want = [(p, zz) for p, zz in want if p is not None]
            assert kxy.tolist() == [[float(p[0]), float(p[1])] for p, _ in want] and kz.tolist() == [zz for _, zz in want], (pyramid is None, l)
            assert 0 < len(kz) < n
    with_clear = pref.keypoints([(xy, z)], L, h, w, BORDERS, [clear])[1]
    without = pref.keypoints([(xy, z)], L, h, w, BORDERS)[1]
    assert (with_clear <= without).all() and with_clear[0, 0] < without[0, 0]
