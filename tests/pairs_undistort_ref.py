"""numpy restatement of the undistortion of include/mbavo.h (mbavo_camera_radtan, mbavo_undistort_map, mbavo_undistort_u8,
mbavo_pairs_opts.undistort): the map, the bilinear remap and the nearest raw position of a depth look-up.  float64 arithmetic in
the order written there, then np.float32; numpy's float64 division is IEEE and nothing here can be contracted into a fused
multiply-add.  tests/test_pairs_undistort_api.py pins its witnesses on the CPU; tests/test_gpu_pairs_undistort.py holds the device
to these functions bit for bit."""
import numpy as np

import pairs_depth_ref as zref

# the three coefficient sets (k1, k2, p1, p2) of the tests: a lens whose corners point outside the raw image, one that stays
# inside, and no distortion
DIST_OUTSIDE = (0.2624, -0.9531, -0.0054, 0.0026)
DIST_INSIDE = (-0.28, 0.07, 2e-4, -1e-4)
DIST_NONE = (0.0, 0.0, 0.0, 0.0)


def intrinsics(H, W):
    """The tests' camera at H x W: fx = 517.3 W / 640, fy = 516.5 W / 640, cx = (W - 1) / 2 + 0.3, cy = (H - 1) / 2 - 0.2."""
    return (517.3 * W / 640, 516.5 * W / 640, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2)


def undistort_map(from_intr, dist, to_intr, H, W):
    """H x W x 2 float32 [sx, sy]: where every pixel of the undistorted `to` camera lies in the raw image."""
    fx_to, fy_to, cx_to, cy_to = (np.float64(v) for v in to_intr)
    fx, fy, cx, cy = (np.float64(v) for v in from_intr)
    k1, k2, p1, p2 = (np.float64(v) for v in dist)
    c, r = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    xn, yn = np.broadcast_to((c - cx_to) / fx_to, (H, W)), np.broadcast_to((r - cy_to) / fy_to, (H, W))
    x, y = (xn * 1.0) / (1.0 + 1e-8), (yn * 1.0) / (1.0 + 1e-8)
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    xd = x + x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
    yd = y + y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
    return np.stack([(fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)], 2)


def usable(map_xy):
    """Entries that point somewhere: finite and below 2^30 in magnitude."""
    with np.errstate(invalid="ignore"):
        return (np.abs(map_xy[..., 0].astype(np.float64)) < 2.0 ** 30) & (np.abs(map_xy[..., 1].astype(np.float64)) < 2.0 ** 30)


def _taps(map_xy):
    ok = usable(map_xy)
    X, Y = (np.where(ok, map_xy[..., i].astype(np.float64), 0.0) for i in (0, 1))
    x0, y0 = np.floor(X), np.floor(Y)
    return ok, x0.astype(np.int64), y0.astype(np.int64), X - x0, Y - y0


def remap_u8(src, map_xy):
    """The Hs x Ws uint8 image through an H x W x 2 map: H x W uint8, 0 outside the raw image."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and map_xy.dtype == np.float32
    Hs, Ws = src.shape
    ok, x0, y0, ax, ay = _taps(map_xy)

    def p(y, x):
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        return np.where(inside, src[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)].astype(np.float64), 0.0)

    v = (1.0 - ay) * ((1.0 - ax) * p(y0, x0) + ax * p(y0, x0 + 1)) + ay * ((1.0 - ax) * p(y0 + 1, x0) + ax * p(y0 + 1, x0 + 1))
    return np.where(ok, (v + 0.5).astype(np.int64), 0).astype(np.uint8)


def tap_outside(map_xy, Hs, Ws):
    """H x W bool: one of the four taps of the pixel lies outside the Hs x Ws raw image (or its entry points nowhere)."""
    ok, x0, y0, _, _ = _taps(map_xy)
    return ~ok | (x0 < 0) | (x0 + 1 >= Ws) | (y0 < 0) | (y0 + 1 >= Hs)


def nearest_raw(map_xy, Hs, Ws):
    """(inside H x W bool, xr, yr): the raw pixel floor(s + 0.5) of every entry and whether it exists."""
    ok = usable(map_xy)
    xr = np.floor(np.where(ok, map_xy[..., 0].astype(np.float64), -1.0) + 0.5).astype(np.int64)
    yr = np.floor(np.where(ok, map_xy[..., 1].astype(np.float64), -1.0) + 0.5).astype(np.int64)
    return ok & (xr >= 0) & (xr < Ws) & (yr >= 0) & (yr < Hs), xr, yr


def depth_through_map(depth_format, raw, map_xy, to_intr, depth_unit=0.0, depth_max=0.0):
    """mbavo_pairs_opts.undistort = 2: the float32 z every level-0 pixel (x0, y0) of the undistorted image is given -- the raw
    element nearest to its map entry through the format's formula (format 1: with the ray of (x0, y0)), 0 where there is none."""
    raw = np.asarray(raw)
    Hs, Ws = raw.shape
    H, W = map_xy.shape[:2]
    inside, xr, yr = nearest_raw(map_xy, Hs, Ws)
    v = raw[np.clip(yr, 0, Hs - 1), np.clip(xr, 0, Ws - 1)]  # H x W elements in the undistorted geometry
    z = zref.to_z(depth_format, np.ascontiguousarray(v), to_intr, depth_unit, depth_max)
    return np.where(inside, z, np.float32(0))
