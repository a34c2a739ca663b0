"""numpy restatement of the clearance mask of include/mbavo.h (mbavo_pairs_opts.valid_radius, mbavo_undistort_clearance_batch):
"valid at level 0", "valid at level l" and "clear at radius r", first as brute-force loops that read like the definitions, then
with cumulative sums for the larger shapes.  tests/test_pairs_valid_api.py holds the two to each other on the CPU;
tests/test_gpu_pairs_valid.py holds the device to them byte for byte.  Everything is integer or comparison logic: exact.

It builds on tests/pairs_undistort_ref.py (undistort_map, DIST_OUTSIDE, tap_outside) and tests/pairs_cameras_ref.py (the unified
map) and names the two cameras the GPU tests use: 50 x 70 undistorted images of a 60 x 80 raw camera under a `to` camera wide
enough that a good part of the image is black margin."""
import numpy as np

import pairs_cameras_ref as cref
import pairs_undistort_ref as uref

H, W, HS, WS, L = 50, 70, 60, 80, 3
# the undistorted pinhole camera of both: a short focal length, so that the 50 x 70 view reaches past the raw image
TO_INTR = (38.0, 37.5, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2)
CAMERAS = {
    # a radial-tangential camera whose corners point outside the raw image
    "radtan": dict(model=1, Hs=HS, Ws=WS, from_intr=uref.intrinsics(HS, WS), xi=0.0, dist=uref.DIST_OUTSIDE, to_intr=TO_INTR),
    # a unified camera with xi = 1: the view narrows towards the edge, the margin's outline is an oval
    "unified": dict(model=2, Hs=HS, Ws=WS, from_intr=(110.0, 109.0, (WS - 1) / 2 - 0.4, (HS - 1) / 2 + 0.3), xi=1.0, dist=(0.0, 0.0, 0.0, 0.0),
                    to_intr=(33.0, 32.5, (W - 1) / 2 - 0.2, (H - 1) / 2 + 0.1)),
}


def camera_map(cam, h=H, w=W):
    """The h x w x 2 float32 map of one of CAMERAS (either model)."""
    return cref.maps_of([cam], h, w)[0]


def valid0(map_xy, Hs, Ws):
    """H x W bool: 0.0 <= X <= Ws - 1 and 0.0 <= Y <= Hs - 1 in double; NaN and +-inf fail, -0.0 passes."""
    X, Y = map_xy[..., 0].astype(np.float64), map_xy[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (0.0 <= X) & (X <= np.float64(Ws - 1)) & (0.0 <= Y) & (Y <= np.float64(Hs - 1))


def level_sizes(h, w, levels):
    return [(h >> l, w >> l) for l in range(levels)]


def pyramid_bytes(h, w, levels):
    return sum(a * b for a, b in level_sizes(h, w, levels))


# ---- the definitions, as loops
def valid_level_loops(v0, l):
    h, w = v0.shape[0] >> l, v0.shape[1] >> l
    out = np.zeros((h, w), bool)
    s = 1 << l
    for y in range(h):
        for x in range(w):
            ok = True
            for j in range(s):
                for i in range(s):
                    ok = ok and bool(v0[y * s + j, x * s + i])
            out[y, x] = ok
    return out


def clear_loops(valid, r):
    h, w = valid.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            ok = True
            for yy in range(y - r, y + r + 1):
                for xx in range(x - r, x + r + 1):
                    ok = ok and 0 <= yy < h and 0 <= xx < w and bool(valid[yy, xx])
            out[y, x] = ok
    return out


def clearance_loops(v0, levels, r):
    """[level 0, .., level levels-1] uint8, by the loops above."""
    return [clear_loops(valid_level_loops(v0, l), r).astype(np.uint8) for l in range(levels)]


# ---- the same with sums
def valid_level(v0, l):
    s = 1 << l
    h, w = v0.shape[0] >> l, v0.shape[1] >> l
    return v0[:h * s, :w * s].reshape(h, s, w, s).all(axis=(1, 3))


def clear(valid, r):
    h, w = valid.shape
    out = np.zeros((h, w), bool)
    if h <= 2 * r or w <= 2 * r:
        return out
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(valid.astype(np.int64), 0), 1)
    n = 2 * r + 1
    box = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]  # windows that lie inside the level
    out[r:h - r, r:w - r] = box == n * n
    return out


def clearance(v0, levels, r):
    """[level 0, .., level levels-1] uint8."""
    return [clear(valid_level(v0, l), r).astype(np.uint8) for l in range(levels)]


def packed(levels_list):
    """The levels one behind the other without padding: the layout of mbavo_undistort_clearance_batch."""
    return np.concatenate([a.ravel() for a in levels_list]).astype(np.uint8)


def handcrafted_map(h=H, w=W, Hs=HS, Ws=WS):
    """An h x w map inside the raw image everywhere but for planted entries: NaN, +inf, -inf, -0.0, exactly 0, exactly Ws - 1 and
    Hs - 1, nextafter on both sides of all four limits, and 2^31 -- scattered so that they fall into different boxes of the
    pyramid.  Returns (map, {(row, col): expected level-0 validity})."""
    m = np.empty((h, w, 2), np.float32)
    m[..., 0], m[..., 1] = np.float32(Ws / 2), np.float32(Hs / 2)
    f, inf, nan = np.float32, np.float32(np.inf), np.float32(np.nan)
    up = lambda v: np.nextafter(f(v), inf)
    down = lambda v: np.nextafter(f(v), -inf)
    plant = [((nan, f(3)), False), ((f(3), nan), False), ((inf, f(3)), False), ((f(3), -inf), False), ((f(-0.0), f(-0.0)), True),
             ((f(0), f(0)), True), ((f(Ws - 1), f(Hs - 1)), True), ((up(Ws - 1), f(1)), False), ((down(Ws - 1), f(1)), True),
             ((f(1), up(Hs - 1)), False), ((f(1), down(Hs - 1)), True), ((down(0), f(1)), False), ((up(0), f(1)), True),
             ((f(1), down(0)), False), ((f(1), up(0)), True), ((f(2.0 ** 31), f(1)), False), ((f(1), f(2.0 ** 31)), False),
             ((f(-2.0 ** 31), f(1)), False)]
    want = {}
    for k, (entry, ok) in enumerate(plant):
        r, c = (5 + 11 * k) % (h - 2), (7 + 17 * k) % (w - 2)  # distinct positions; the last row and column (no box) stay plain
        assert (r, c) not in want
        m[r, c] = entry
        want[(r, c)] = ok
    m[h - 1, w - 1] = (nan, nan)  # (50 x 70: a pixel that belongs to no box of level 2)
    want[(h - 1, w - 1)] = False
    return m, want
