"""mbavo_pairs_carry_save / mbavo_pairs_carry_adopt without a GPU: the entries exist in the library, the header and the binding, the
structs have the sizes the header states, NULL handles are rejected -- and the specification, restated in numpy
(tests/pairs_carry_ref.py, brute force), is held to hand-made cases and to two keyframes of a workloads.RenderedScene.

The property is established HERE (the figures are in profiles/r34_pairs_carry.txt): keyframe A's keypoints carry the plane's exact
depths, keyframe B's are prepared at a constant wrong depth, T comes from the scene's true poses.  Every keypoint of B that adopts
takes a mean of inverse depths of plane points whose pixels lie within radius of its own, so within radius + 0.5 pixels of it before
rounding: its relative depth error is bounded by (radius + 1) pixels times the plane's analytic relative depth change per pixel in B
(pairs_carry_ref.plane_gradient), the half pixel left over covering the change of that gradient across the window.  The share that
adopts is bounded from below by pairs_carry_ref.property_share_bound's reasoning.  tests/test_gpu_pairs_carry.py asserts the same
bound on the device's depths and the restatement's share.  Every test here asks the library for the calls first: none passes where
they do not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_carry_ref as cref

E_ARG = -1
NEW = ["mbavo_pairs_carry_save_opts_size", "mbavo_pairs_carry_save_size", "mbavo_pairs_carry_adopt_opts_size", "mbavo_pairs_carry_adopt_size",
       "mbavo_pairs_carry_save", "mbavo_pairs_carry_adopt", "mbavo_pairs_carry_save_stats", "mbavo_pairs_carry_adopt_stats"]
INTR = (32.0, 32.0, 32.0, 24.0)
W, H = 64, 48
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


@pytest.fixture(autouse=True)
def the_calls_exist(mbavo):
    """The restatement restates calls of the library: its records are the binding's."""
    lib = mbavo.load()
    assert lib.mbavo_pairs_carry_save_size() == C.sizeof(mbavo.capi.PairsCarrySave)
    assert lib.mbavo_pairs_carry_adopt_size() == C.sizeof(mbavo.capi.PairsCarryAdopt)


def test_entries_and_struct_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS and name in header
    assert lib.mbavo_pairs_carry_save_opts_size() == C.sizeof(capi.PairsCarrySaveOpts) == 8 + 3 * 8 + 16
    assert lib.mbavo_pairs_carry_save_size() == C.sizeof(capi.PairsCarrySave) == 16 + 8
    assert lib.mbavo_pairs_carry_adopt_opts_size() == C.sizeof(capi.PairsCarryAdoptOpts) == 16 + 5 * 8 + 16
    assert lib.mbavo_pairs_carry_adopt_size() == C.sizeof(capi.PairsCarryAdopt) == 16 + 2 * 8
    # the header's own figures, on the lines that open the four structs
    assert "typedef struct mbavo_pairs_carry_save_opts { /* zero-initialise; 48 bytes, no padding */" in header
    assert "struct mbavo_pairs_carry_save {            /* one per (listed pair, level); 24 bytes, no padding */" in header
    assert "typedef struct mbavo_pairs_carry_adopt_opts { /* zero-initialise; 72 bytes, no padding */" in header
    assert "struct mbavo_pairs_carry_adopt {           /* one per (listed pair, level); 32 bytes, no padding */" in header


def test_null_handles_are_rejected(mbavo):
    """(each bad argument of a live object: tests/test_gpu_pairs_carry.py, an object needs a device)"""
    lib, capi = mbavo.load(), mbavo.capi
    assert cref.call_save(lib, None, [0], IDENTITY, cref.save_opts(capi), (capi.PairsCarrySave * 4)()) == E_ARG
    assert cref.call_adopt(lib, None, [0], cref.adopt_opts(capi), (capi.PairsCarryAdopt * 4)()) == E_ARG
    assert lib.mbavo_pairs_carry_save_stats(None, (C.c_longlong * 3)()) == E_ARG
    assert lib.mbavo_pairs_carry_adopt_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert all(callable(getattr(workloads.PairBatch, n)) for n in ("carry_save", "carry_adopt", "carry_stats"))


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def test_identity_hands_every_point_to_itself(mbavo):
    """Identity T, radius 1, points 3 pixels apart: every point's window holds its own carried point alone.  D -> 1 / D -> (1 (1 /
    D)) / 1 -> 1 / (1 / D): two roundings of a reciprocal, at most 2 ulp."""
    rng = np.random.default_rng(1)
    ys, xs = np.meshgrid(np.arange(1, H, 3), np.arange(2, W, 3), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    z = rng.uniform(0.5, 9.0, len(xy))
    s = cref.save(xy, z, INTR, W, H, IDENTITY)
    assert s["carried"].all() and np.array_equal(s["px"], xy.astype(np.int64)) and (s["w"] == 1.0).all() and s["sum_w"] == len(xy)
    m = cref.adopt(xy, np.full(len(xy), 3.0), s, 1)
    assert (m["flags"] == cref.ADOPTED).all() and (m["count"] == 1).all() and m["num_adopted"] == len(xy) and m["num_empty"] == 0
    assert _ulps(m["z_new"], z).max() <= 2
    assert (m["info"] == 1.0).all() and m["sum_info"] == len(xy)


def test_a_translation_along_z_scales_the_weight_by_the_closed_form(mbavo):
    """T = (0, 0, tz): D' = D - tz, c = 1, s = D^2 / D'^2, so w' = deflate (D' / D)^4 -- three divisions and three products away:
    within 8 ulp.  The pixel moves away from the principal point by D / D'."""
    xy = np.array([[40.0, 30.0], [32.0, 24.0], [10.0, 5.0], [63.0, 47.0]])
    z = np.array([2.0, 3.0, 5.0, 4.0])
    tz, deflate = 0.5, 0.75
    s = cref.save(xy, z, INTR, W, H, np.array([0, 0, tz, 0, 0, 0, 1.0]), deflate=deflate)
    Dn = z - tz
    assert s["carried"].tolist() == [True, True, True, False]  # (63, 47) leaves the image: dropped, not clamped
    assert np.array_equal(s["D_new"], Dn) and np.array_equal(s["rho"][:3], 1.0 / Dn[:3])
    assert _ulps(s["w"][:3], deflate * (Dn[:3] / z[:3]) ** 4).max() <= 8
    want = np.floor((xy - [32.0, 24.0]) * (z / Dn)[:, None] + [32.0, 24.0] + 0.5)
    assert np.array_equal(s["px"][:3], want[:3].astype(np.int64)) and s["px"][3].tolist() == [-1, -1]
    # the filter's info as the weight, a zero and a NaN among them: dropped
    s = cref.save(xy[:3], z[:3], INTR, W, H, np.array([0, 0, tz, 0, 0, 0, 1.0]), w=[4.0, 0.0, float("nan")])
    assert s["carried"].tolist() == [True, False, False] and _ulps(s["w"][0], 4.0 * (1.5 / 2.0) ** 4) <= 8
    # behind the new camera, and closer than z_min
    s = cref.save(xy[:2], [0.4, 0.505], INTR, W, H, np.array([0, 0, tz, 0, 0, 0, 1.0]))
    assert s["carried"].tolist() == [False, False] and s["num_valid"] == 2 and s["num_carried"] == 0


def test_the_foreground_rule_keeps_the_near_surface(mbavo):
    """Two layers over the same pixels, 2.0 in front of 3.0: with max_rel_diff = 0.1 the far layer (rho 0.33 < 0.9 x 0.5) stays out
    of every sum; with max_rel_diff = 1 both enter."""
    ys, xs = np.meshgrid(np.arange(10, 16), np.arange(10, 16), indexing="ij")
    near = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    far = np.concatenate([near, near + [6.0, 0.0]])  # the far layer reaches further right
    xy = np.concatenate([near, far])
    z = np.concatenate([np.full(len(near), 2.0), np.full(len(far), 3.0)])
    s = cref.save(xy, z, INTR, W, H, IDENTITY)
    new = np.array([[12.0, 12.0], [15.0, 12.0], [20.0, 12.0], [40.0, 40.0]])
    m = cref.adopt(new, np.full(4, 9.0), s, 1, max_rel_diff=0.1)
    assert m["flags"].tolist() == [1, 1, 1, 0] and m["count"].tolist() == [9, 6, 9, 0]
    assert m["z_new"].tolist() == [2.0, 2.0, 3.0, 9.0] and np.isnan(m["rho"][3]) and m["info"][3] == 0
    both = cref.adopt(new, np.full(4, 9.0), s, 1, max_rel_diff=1.0)
    # ((15, 12): the near layer ends at x = 15, the far one goes on)
    assert both["count"].tolist() == [18, 6 + 9, 9, 0] and 2.0 < both["z_new"][0] < 3.0
    # min_support and the limits
    m = cref.adopt(new, np.full(4, 9.0), s, 1, min_support=7)
    assert m["flags"].tolist() == [1, 2, 1, 0] and m["z_new"][1] == 9.0
    m = cref.adopt(new, np.full(4, 9.0), s, 1, z_min=2.5)
    assert m["flags"].tolist() == [3, 3, 1, 0] and m["count"].tolist() == [9, 6, 9, 0] and m["num_adopted"] == 1 and m["num_empty"] == 1
    # the seed: adopted keypoints take rho_n and the capped SW, the others the filter's own seed of their depth
    m = cref.adopt(new, np.full(4, 9.0), s, 1, prior_rel_sigma=0.5, max_info=4.0)
    assert m["mu"].tolist() == [0.5, 0.5, 1.0 / 3.0, 1.0 / 9.0] and m["info_state"][:3].tolist() == [4.0, 4.0, 4.0]
    assert m["info_state"][3] == 1.0 / ((0.5 * (1.0 / 9.0)) * (0.5 * (1.0 / 9.0)))


def test_the_sums_run_over_ascending_source_index(mbavo):
    """1 + 2^-53 + 2^-53 left to right stays 1; 2^-53 + 2^-53 + 1 is 1 + 2^-52."""
    tiny = 2.0 ** -53
    xy = np.array([[5.0, 5.0], [6.0, 5.0], [5.0, 6.0]])
    s = cref.save(xy, np.full(3, 2.0), INTR, W, H, IDENTITY, w=[1.0, tiny, tiny])
    m = cref.adopt([[5.0, 5.0]], [9.0], s, 1)
    back = cref.adopt([[5.0, 5.0]], [9.0], s, 1, order=lambda js: js[::-1])
    assert m["info"][0] == 1.0 and back["info"][0] == 1.0 + 2.0 ** -52


def test_record_sums_follow_the_grid(mbavo):
    """Keypoints 0 and 256 share lane 0 of workgroup 0 when the capacity is one tile, and meet only in the last sum when it is two."""
    t = np.zeros(300)
    t[0], t[1], t[256] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert cref.record_sum(t, 256) == 1.0            # lane 0: (1 + 2^-53) = 1, then + lane 1's 2^-53: 1
    assert cref.record_sum(t[:257], 512) == 1.0      # two workgroups: 1 + 2^-53
    t[1] = 0.0
    t[257] = 2.0 ** -53
    assert cref.record_sum(t, 512) == 1.0 + 2.0 ** -52  # workgroup 1 holds 2^-53 + 2^-53 = 2^-52


def test_property_two_keyframes_of_a_rendered_scene(mbavo):
    scene = cref.property_scene(mbavo.load(), mbavo.capi)
    r = cref.PROPERTY["radius"]
    s = cref.save(*scene["A"], scene["intr"], scene["W"], scene["H"], scene["T"])
    m = cref.adopt(*scene["B"], s, **cref.PROPERTY)
    share, worst = cref.property_figures(scene, m, r)
    bound = cref.property_share_bound(scene, r)
    print("shift %.2f px; carried %d of %d; adopted share %.4f (bound %.4f); largest error / ((radius + 1) gradient) = %.3f; gradient %.2e .. %.2e per px"
          % (scene["shift"], s["num_carried"], s["num_keypoints"], share, bound, worst, scene["grad"].min(), scene["grad"].max()))
    assert scene["shift"] > 1.0  # (the two keyframes are apart: the warp does something)
    assert share >= bound > 0.5
    assert worst <= 1.0
