"""numpy restatement of the caller's keypoints of include/mbavo.h (mbavo_pairs_prepare_points, _update_points): a level-0 point
(x0, y0, z) taken to level l, the tests that keep or drop it there, and the ordered lists of a (pair, level) -- once point by point
as the header reads (kept_at) and once over whole lists (level_keypoints).  tests/test_pairs_points_api.py holds the two to each other
and to hand-made edge cases on the CPU; tests/test_gpu_pairs_points.py holds the device to them bit for bit.  Comparisons, a
division by a power of two and one floor: exact.  The clearance pyramids are tests/pairs_valid_ref.py's and
tests/pairs_mask_ref.py's, as lists [level 0, .., level L-1] of uint8 images."""
import math

import numpy as np

LIMIT = 2.0 ** 30


# ---- the definition, one point at a time
def kept_at(x0, y0, z, l, Hl, Wl, m, clear_l=None):
    """None where the point is dropped at level l (Hl x Wl, border m, optional clearance image of that level), else (xi, yi)."""
    s = float(1 << l)
    xl, yl = float(x0) / s, float(y0) / s
    if not (abs(xl) < LIMIT and abs(yl) < LIMIT):  # (NaN and +-inf fail)
        return None
    xi, yi = int(math.floor(xl + 0.5)), int(math.floor(yl + 0.5))
    z = float(z)
    if z < 1e-2 or not math.isfinite(z):
        return None
    if not (xi >= m and xi < Wl - m and yi >= m and yi < Hl - m):
        return None
    if clear_l is not None and clear_l[yi, xi] == 0:
        return None
    return xi, yi


# ---- the same over a list
def level_keypoints(xy, z, l, Hl, Wl, m, clear_l=None):
    """(kp_xy k x 2 float64, kp_z k float64): the kept points of the list in the list's order; z is the caller's double."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z = np.asarray(z, np.float64).reshape(-1)
    s = np.float64(1 << l)
    with np.errstate(invalid="ignore", over="ignore"):
        xl, yl = xy[:, 0] / s, xy[:, 1] / s
        usable = (np.abs(xl) < LIMIT) & (np.abs(yl) < LIMIT)
        xi = np.floor(np.where(usable, xl, 0.0) + 0.5).astype(np.int64)
        yi = np.floor(np.where(usable, yl, 0.0) + 0.5).astype(np.int64)
        keep = usable & ~(z < 1e-2) & np.isfinite(z)
    keep &= (xi >= m) & (xi < Wl - m) & (yi >= m) & (yi < Hl - m)
    if clear_l is not None:
        inside = (xi >= 0) & (xi < Wl) & (yi >= 0) & (yi < Hl)
        keep &= inside & (clear_l[np.where(inside, yi, 0), np.where(inside, xi, 0)] != 0)
    return np.stack([xi[keep], yi[keep]], 1).astype(np.float64).reshape(-1, 2), z[keep].copy()


def keypoints(points, L, H, W, borders, clear_of_pair=None):
    """points: one (xy, z) per pair.  Returns (per (pair, level), pair-major, dict(xy, z); counts B x L int32).  clear_of_pair: per pair
    the clearance pyramid of its camera, or None."""
    out, counts = [], np.zeros((len(points), L), np.int32)
    for b, (xy, z) in enumerate(points):
        for l in range(L):
            clear_l = None if clear_of_pair is None else clear_of_pair[b][l]
            kxy, kz = level_keypoints(xy, z, l, H >> l, W >> l, borders[l], clear_l)
            out.append(dict(xy=kxy, z=kz))
            counts[b, l] = len(kz)
    return out, counts


def edge_points(H, W, borders, z=1.5):
    """Hand-made level-0 points with what becomes of them, [(x0, y0, z, {level: kept})] for the levels of `borders`: the rounding at
    -0.5 and at W - 0.5, depths on both sides of 1e-2, values that are no number or too large, a point inside level 0's border band
    that level 2 keeps, and two points that share a level-2 pixel."""
    L = len(borders)
    mid_x, mid_y = float(4 * (W // 8)), float(4 * (H // 8))  # whole pixels on every level up to 2, far from every band
    every, none = {l: True for l in range(L)}, {l: False for l in range(L)}
    nan, inf = float("nan"), float("inf")
    pts = [
        (-0.5, mid_y, z, {l: borders[l] == 0 for l in range(L)}),           # floor(-0.5 + 0.5) = 0: pixel 0, kept where the border is 0
        (W - 0.5, mid_y, z, {0: False}),                                    # pixel W at level 0: outside (the coarser levels depend on W)
        (mid_x, mid_y, 0.01, every), (mid_x, mid_y, 0.0099, none),          # !(z < 1e-2)
        (mid_x, mid_y, 0.0, none), (mid_x, mid_y, -1.0, none),
    ]
    for bad in (nan, inf, -inf, 1e300, -1e300):
        pts += [(bad, mid_y, z, none), (mid_x, bad, z, none)]
    for bad in (nan, inf, -inf):
        pts.append((mid_x, mid_y, bad, none))
    pts.append((mid_x, mid_y, 1e300, every))                                # a finite depth that passes !(z < 1e-2): kept, unchanged
    pts.append((2.0 ** 31, mid_y, z, none))
    pts.append((-(2.0 ** 31) - 0.5, mid_y, z, none))
    return pts
