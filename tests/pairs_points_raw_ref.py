"""numpy restatement of the inverse camera of include/mbavo.h (mbavo_undistort_points_batch, mbavo_pairs_set_points_geometry): a raw
pixel (u, v) of a camera of either model into the undistorted image -- once point by point as the header reads (inverse_point) and
once over arrays (inverse), with np.float32 where the header says `float`.  float64 arithmetic in the order written there; numpy's
division and square roots are IEEE (correctly rounded) and nothing here can be contracted into a fused multiply-add.  It also holds
the raw-bounds test of a pairs batch's raw points and the composition with tests/pairs_points_ref.py, and the forward entry of
tests/pairs_undistort_ref.py / pairs_unified_ref.py at real-valued positions for the round trip.
tests/test_pairs_points_raw_api.py holds the two restatements to each other, to the round trip and to hand-made cases on the CPU;
tests/test_gpu_pairs_points_raw.py holds the device to them bit for bit.

A camera is a dict as in tests/pairs_cameras_ref.py: model, Hs, Ws, from_intr, xi, dist, to_intr."""
import numpy as np

import pairs_points_ref as pref

STEPS, STOP = 5, 1e-15
SCALE = 1.0 + 1e-8  # CameraPinhole.cpp:30-31, as the map divides by it


def _f64(values):
    return tuple(np.float64(v) for v in values)


# ---- the forward direction at real-valued positions (float64, before the map's conversion to float)
def forward(cam, X, Y):
    """Where position (X, Y) of the undistorted image lies in the raw image: the entry of pairs_undistort_ref.undistort_map (model
    1) or pairs_unified_ref.undistort_map (model 2) with (X, Y) in place of the pixel grid, (sx, sy) in float64."""
    fx_to, fy_to, cx_to, cy_to = _f64(cam["to_intr"])
    fx, fy, cx, cy = _f64(cam["from_intr"])
    k1, k2, p1, p2 = _f64(cam["dist"])
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    xn, yn = (X - cx_to) / fx_to, (Y - cy_to) / fy_to
    if cam["model"] == 2:
        xi = np.float64(cam["xi"])
        Xc, Yc = xn * 1.0, yn * 1.0
        d = np.sqrt(Xc * Xc + Yc * Yc + 1.0)
        rz = 1.0 / (1.0 + xi * d)
        x, y = Xc * rz, Yc * rz
    else:
        x, y = (xn * 1.0) / (1.0 + 1e-8), (yn * 1.0) / (1.0 + 1e-8)
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    xd = x + x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
    yd = y + y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
    return fx * xd + cx, fy * yd + cy


# ---- the definition, one point at a time
def undistort_normalised(dist, px, py):
    """DistortionRadTan::undistort at p: (qx, qy, solved, steps taken)."""
    k1, k2, p1, p2 = _f64(dist)
    px, py = np.float64(px), np.float64(py)
    qx, qy = px, py
    stopped, steps = False, 0
    with np.errstate(all="ignore"):
        while steps < STEPS and not stopped:
            mx2, my2, mxy = qx * qx, qy * qy, qx * qy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            dx = qx + qx * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
            dy = qy + qy * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
            J00 = 1.0 + rad + 2.0 * k1 * mx2 + 4.0 * k2 * mx2 * rho2 + 2.0 * p1 * qy + 6.0 * p2 * qx
            J01 = 2.0 * k1 * mxy + 4.0 * k2 * rho2 * mxy + 2.0 * p1 * qx + 2.0 * p2 * qy
            J10 = J01
            J11 = 1.0 + rad + 2.0 * k1 * my2 + 4.0 * k2 * my2 * rho2 + 2.0 * p2 * qx + 6.0 * p1 * qy
            ex, ey = px - dx, py - dy
            a, b, c = J00 * J00 + J10 * J10, J00 * J01 + J10 * J11, J01 * J01 + J11 * J11
            g0, g1 = J00 * ex + J10 * ey, J01 * ex + J11 * ey
            det = a * c - b * b
            qx, qy = qx + (c * g0 - b * g1) / det, qy + (a * g1 - b * g0) / det
            steps += 1
            stopped = bool(ex * ex + ey * ey < STOP)
    return qx, qy, stopped and bool(np.isfinite(qx)) and bool(np.isfinite(qy)), steps


def inverse_point(cam, u, v):
    """(X, Y, ok) of one raw pixel; (nan, nan, False) where there is no solution."""
    fx_to, fy_to, cx_to, cy_to = _f64(cam["to_intr"])
    fx, fy, cx, cy = _f64(cam["from_intr"])
    u, v = np.float64(u), np.float64(v)
    with np.errstate(all="ignore"):
        qx, qy, ok, _ = undistort_normalised(cam["dist"], (u - cx) / fx, (v - cy) / fy)
        x, y = qx, qy
        if cam["model"] == 2:
            xi = np.float64(cam["xi"])
            rho2 = np.float32(qx * qx + qy * qy)
            beta = np.float32(1.0 + (1.0 - xi * xi) * np.float64(rho2))
            lam = np.float32((xi + np.float64(np.sqrt(beta))) / (1.0 + np.float64(rho2)))
            pz = np.float64(lam) - xi
            if beta < 0 or pz < 0:
                ok = False
            x, y = (np.float64(lam) * qx) / pz, (np.float64(lam) * qy) / pz
        X, Y = fx_to * (x * SCALE) + cx_to, fy_to * (y * SCALE) + cy_to
    ok = ok and bool(np.isfinite(X)) and bool(np.isfinite(Y))
    return (X, Y, True) if ok else (np.float64("nan"), np.float64("nan"), False)


# ---- the same over arrays
def inverse(cam, uv, want_steps=False):
    """(xy n x 2 float64, ok n uint8) of the raw pixels uv (n x 2); NaN rows where there is no solution.  want_steps: also the
    number of steps every point took."""
    fx_to, fy_to, cx_to, cy_to = _f64(cam["to_intr"])
    fx, fy, cx, cy = _f64(cam["from_intr"])
    k1, k2, p1, p2 = _f64(cam["dist"])
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        px, py = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
        qx, qy = px.copy(), py.copy()
        stopped, steps = np.zeros(len(px), bool), np.zeros(len(px), np.int32)
        for _ in range(STEPS):
            mx2, my2, mxy = qx * qx, qy * qy, qx * qy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            dx = qx + qx * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
            dy = qy + qy * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
            J00 = 1.0 + rad + 2.0 * k1 * mx2 + 4.0 * k2 * mx2 * rho2 + 2.0 * p1 * qy + 6.0 * p2 * qx
            J01 = 2.0 * k1 * mxy + 4.0 * k2 * rho2 * mxy + 2.0 * p1 * qx + 2.0 * p2 * qy
            J10 = J01
            J11 = 1.0 + rad + 2.0 * k1 * my2 + 4.0 * k2 * my2 * rho2 + 2.0 * p2 * qx + 6.0 * p1 * qy
            ex, ey = px - dx, py - dy
            a, b, c = J00 * J00 + J10 * J10, J00 * J01 + J10 * J11, J01 * J01 + J11 * J11
            g0, g1 = J00 * ex + J10 * ey, J01 * ex + J11 * ey
            det = a * c - b * b
            live = ~stopped
            qx = np.where(live, qx + (c * g0 - b * g1) / det, qx)
            qy = np.where(live, qy + (a * g1 - b * g0) / det, qy)
            steps += live
            stopped |= live & (ex * ex + ey * ey < STOP)
        ok = stopped & np.isfinite(qx) & np.isfinite(qy)
        x, y = qx, qy
        if cam["model"] == 2:
            xi = np.float64(cam["xi"])
            rho2 = (qx * qx + qy * qy).astype(np.float32)
            beta = (1.0 + (1.0 - xi * xi) * rho2.astype(np.float64)).astype(np.float32)
            lam = ((xi + np.sqrt(beta).astype(np.float64)) / (1.0 + rho2.astype(np.float64))).astype(np.float32)
            pz = lam.astype(np.float64) - xi
            ok &= ~(beta < 0) & ~(pz < 0)
            x, y = (lam.astype(np.float64) * qx) / pz, (lam.astype(np.float64) * qy) / pz
        X, Y = fx_to * (x * SCALE) + cx_to, fy_to * (y * SCALE) + cy_to
        ok &= np.isfinite(X) & np.isfinite(Y)
    xy = np.stack([np.where(ok, X, np.nan), np.where(ok, Y, np.nan)], 1)
    return (xy, ok.astype(np.uint8), steps) if want_steps else (xy, ok.astype(np.uint8))


# ---- a pairs batch's raw points
def raw_inside(uv, Hs, Ws):
    """n bool: 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1 in double; NaN and +-inf fail, -0.0 passes."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return (0.0 <= uv[:, 0]) & (uv[:, 0] <= np.float64(Ws - 1)) & (0.0 <= uv[:, 1]) & (uv[:, 1] <= np.float64(Hs - 1))


def to_undistorted(cam, uv):
    """The geometry-0 points of a list of raw points: NaN for a point outside the raw image or without a solution."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    xy, _ = inverse(cam, uv)
    xy[~raw_inside(uv, cam["Hs"], cam["Ws"])] = np.nan
    return xy


def keypoints(points, cam_of_pair, L, H, W, borders, clear_of_pair=None):
    """pairs_points_ref.keypoints of raw lists: points is one (uv, z) per pair, cam_of_pair that pair's camera."""
    return pref.keypoints([(to_undistorted(cam, uv), z) for (uv, z), cam in zip(points, cam_of_pair)], L, H, W, borders, clear_of_pair)


def edge_points(cam):
    """Hand-made raw pixels of a camera, [(u, v)]: the principal point, the raw image's corners and the edges of the bounds test
    (-0.0, Ws - 1, just outside), values that are no number or too large."""
    Hs, Ws = cam["Hs"], cam["Ws"]
    cx, cy = cam["from_intr"][2], cam["from_intr"][3]
    nan, inf = float("nan"), float("inf")
    below, above_w, above_h = np.nextafter(0.0, -1.0), np.nextafter(float(Ws - 1), inf), np.nextafter(float(Hs - 1), inf)
    pts = [(cx, cy), (-0.0, -0.0), (0.0, 0.0), (float(Ws - 1), float(Hs - 1)), (float(Ws - 1), 0.0), (0.0, float(Hs - 1)),
           (below, cy), (cx, below), (above_w, cy), (cx, above_h), (-1.0, cy), (float(Ws), cy), (cx, float(Hs))]
    for bad in (nan, inf, -inf, 1e300, -1e300):
        pts += [(bad, cy), (cx, bad)]
    return pts
