"""A set of cameras in one batch of pairs (include/mbavo.h: mbavo_pairs_camera, mbavo_pairs_set_cameras,
mbavo_undistort_map_batch), restated in numpy.  Nothing new is computed here: a camera's map is that of its model's restatement
(tests/pairs_undistort_ref.py for model 1, tests/pairs_unified_ref.py for model 2) with the camera's own to_intrinsics, and a
pair's expected arrays are those of its camera.  tests/test_pairs_cameras_api.py pins the witnesses of the set below on the CPU;
tests/test_gpu_pairs_cameras.py holds the device to these maps bit for bit."""
import numpy as np

import pairs_undistort_ref as uref
import pairs_unified_ref as xref

GEOMETRIES = {"crop": (48, 64, 52, 76), "odd": (45, 63, 52, 76)}  # H, W of the undistorted images, Hs, Ws of the raw ones
CAMERA_OF_PAIR = (0, 1, 0, 2)  # B = 4, G = 3: pairs 0 and 2 share camera 0, and the indices do not ascend
SWAPPED = (0, 2, 0, 1)         # the cameras of pairs 1 and 3 exchanged


def cameras(geometry):
    """The G = 3 cameras of the tests, as dicts (model, Hs, Ws, from_intr, xi, dist, to_intr):
      0  radial-tangential, the coefficient set that points at taps outside the raw image; the tests' pinhole camera at H x W
      1  unified, the parameter set that stays inside; a pinhole camera a few percent off camera 0's in every entry
      2  radial-tangential with zero coefficients; a third pinhole camera, again off in every entry"""
    H, W, Hs, Ws = GEOMETRIES[geometry]
    K = uref.intrinsics(48, 64)  # ("odd": the same pinhole camera, its image cut to 45 x 63 -- three of the corners stay in view)
    radtan_from = (517.3 * Ws / 640, 1.12 * K[1], (Ws - 1) / 2 + 0.3, (Hs - 1) / 2 - 0.2)  # (tests/test_gpu_pairs_undistort.py: "crop")
    s = xref.SETS["inside"]
    return [
        dict(model=1, Hs=Hs, Ws=Ws, from_intr=radtan_from, xi=0.0, dist=uref.DIST_OUTSIDE, to_intr=K),
        dict(model=2, Hs=Hs, Ws=Ws, from_intr=xref.from_intrinsics("inside", "crop", Hs, Ws), xi=s["xi"], dist=s["dist"],
             to_intr=(1.03 * K[0], 0.98 * K[1], K[2] + 0.4, K[3] - 0.3)),
        dict(model=1, Hs=Hs, Ws=Ws, from_intr=radtan_from, xi=0.0, dist=uref.DIST_NONE, to_intr=(0.95 * K[0], 1.04 * K[1], K[2] - 0.7, K[3] + 0.5)),
    ]


def camera_map(cam, H, W):
    """H x W x 2 float32: the map of one camera, by the restatement of its model."""
    if cam["model"] == 2:
        return xref.undistort_map(cam["from_intr"], cam["xi"], cam["dist"], cam["to_intr"], H, W)
    assert cam["model"] == 1
    return uref.undistort_map(cam["from_intr"], cam["dist"], cam["to_intr"], H, W)


def maps_of(cams, H, W):
    return np.stack([camera_map(c, H, W) for c in cams])


def per_pair(per_camera, camera_of_pair):
    """The per-pair array of something every camera has one of (maps, intrinsics)."""
    return np.stack([np.asarray(per_camera[g]) for g in camera_of_pair])


def remapped(raw, maps, camera_of_pair):
    """Raw images B x Hs x Ws through the map of every pair's camera: B x H x W uint8."""
    return np.stack([uref.remap_u8(im, maps[g]) for im, g in zip(raw, camera_of_pair)])


def level_intrinsics(cams, camera_of_pair, L):
    """B x L x 4: what every entry of the problems array holds, to_intrinsics / (1 << l)."""
    return np.array([[[v / float(1 << l) for v in cams[g]["to_intr"]] for l in range(L)] for g in camera_of_pair], np.float64)
