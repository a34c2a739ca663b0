"""numpy restatement of the unified-camera undistortion map of include/mbavo.h (mbavo_camera_unified,
mbavo_undistort_map_unified): float64 arithmetic in the order written there, then np.float32.  numpy's float64 division and
square root are IEEE (correctly rounded) and nothing here can be contracted into a fused multiply-add.  Everything downstream of
the map is camera-independent and comes unchanged from tests/pairs_undistort_ref.py (remap_u8, nearest_raw, tap_outside,
depth_through_map).  tests/test_pairs_unified_api.py pins the model and the witnesses of the three parameter sets on the CPU;
tests/test_gpu_pairs_unified.py holds the device to these functions bit for bit."""
import numpy as np

import pairs_undistort_ref as uref
from pairs_undistort_ref import depth_through_map, nearest_raw, remap_u8, tap_outside  # noqa: F401  (re-exported, unchanged)

# The three parameter sets of the tests.  A unified camera compresses the image towards its edges (rz falls with the distance
# from the axis), so whether the corners of the undistorted image point outside the raw image is decided by the raw focal
# length: `focal` multiplies fx and fy of the tests' camera (pairs_undistort_ref.intrinsics at the raw size), per geometry of
# tests/test_gpu_pairs_unified.py ("crop": a 52 x 76 sensor into 48 x 64; "same": 50 x 70 into 50 x 70; "wide": as "crop" with a longer focal length, which puts four
# whole rows of the undistorted image outside the raw one, for the depth look-up).  (1 + xi) would keep the
# scale of the image centre.
#   outside: xi about 1 and a k1 that outweighs the mirror's compression at the corners; the focal length pushes the corners (and
#            the rows next to them) of the undistorted image off the raw image
#   inside:  a smaller xi, a distortion of the other sign; every tap stays inside
#   pinhole: xi = 0 and no distortion object -- the affine change of camera, exactly
SETS = {
    "outside": dict(xi=1.05, dist=(0.9, -0.2, 3e-4, -2e-4), focal=dict(crop=2.0, same=2.15, wide=2.1)),
    "inside": dict(xi=0.8, dist=(0.035, -0.006, -2e-4, 1e-4), focal=dict(crop=1.6, same=1.7)),
    "pinhole": dict(xi=0.0, dist=(0.0, 0.0, 0.0, 0.0), focal=dict(crop=1.0, same=1.0)),
}


def intrinsics(H, W):
    return uref.intrinsics(H, W)


def from_intrinsics(name, geometry, Hs, Ws):
    """fx fy cx cy of the raw unified camera of a parameter set at Hs x Ws."""
    fx, fy, cx, cy = uref.intrinsics(Hs, Ws)
    f = SETS[name]["focal"][geometry]
    return (f * fx, f * fy, cx, cy)


def undistort_map(from_intr, xi, dist, to_intr, H, W, dtype=np.float32):
    """H x W x 2 float32 [sx, sy]: where every pixel of the undistorted pinhole `to` camera lies in the raw unified image.
    (dtype=np.float64: the entries before the conversion to float, what the reference's `project` returns.)"""
    fx_to, fy_to, cx_to, cy_to = (np.float64(v) for v in to_intr)
    fx, fy, cx, cy = (np.float64(v) for v in from_intr)
    k1, k2, p1, p2 = (np.float64(v) for v in dist)
    xi = np.float64(xi)
    c, r = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    xn, yn = np.broadcast_to((c - cx_to) / fx_to, (H, W)), np.broadcast_to((r - cy_to) / fy_to, (H, W))
    X, Y = xn * 1.0, yn * 1.0
    d = np.sqrt(X * X + Y * Y + 1.0)
    rz = 1.0 / (1.0 + xi * d)
    x, y = X * rz, Y * rz
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    xd = x + x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
    yd = y + y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
    return np.stack([(fx * xd + cx).astype(dtype), (fy * yd + cy).astype(dtype)], 2)


def affine_grid(from_intr, to_intr, H, W):
    """The closed form of the xi = 0, no-distortion map: sx = (float)(fx_from * xn + cx_from)."""
    fx_to, fy_to, cx_to, cy_to = (np.float64(v) for v in to_intr)
    fx, fy, cx, cy = (np.float64(v) for v in from_intr)
    c, r = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    sx, sy = np.broadcast_to(fx * ((c - cx_to) / fx_to) + cx, (H, W)), np.broadcast_to(fy * ((r - cy_to) / fy_to) + cy, (H, W))
    return np.stack([sx.astype(np.float32), sy.astype(np.float32)], 2)
