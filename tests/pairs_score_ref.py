"""numpy restatement of the corner score (include/mbavo.h: mbavo_corner_score_u8, mbavo_pairs_set_detector), written from the
definition and not from the kernel, and the restated selection: the host detector of the other pairs tests (pairs_ref.keypoints,
pairs_dense_ref.keypoints, pairs_oracle.host_levels) with the response swapped.  Helper, no test in it.

    kx, ky   right - left and bottom - top as integers, zero on the 1-pixel border
    a, b, c  sums of kx^2, kx ky, ky^2 over the (2r+1)^2 window; positions outside the image contribute 0; n = (2r+1)^2 always
    tr = a + c; s = sqrt((a - c)^2 + 4 b^2); d = max(tr - s, 0); score = float32(sqrt(d / (8 n)))      (all in float64)

Every operation is exact or one correctly rounded IEEE operation, so the device's floats equal these bit for bit."""
import contextlib

import numpy as np

import pairs_ref


def differences(img):
    """(kx, ky) as int64 H x W."""
    v = np.asarray(img).astype(np.int64)
    kx, ky = np.zeros_like(v), np.zeros_like(v)
    kx[1:-1, 1:-1] = v[1:-1, 2:] - v[1:-1, :-2]
    ky[1:-1, 1:-1] = v[2:, 1:-1] - v[:-2, 1:-1]
    return kx, ky


def window_sum(p, r):
    """Sum over the (2r+1)^2 window around every pixel of the int64 image p, zeros outside."""
    H, W = p.shape
    q = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    q[r:r + H, r:r + W] = p
    out = np.zeros((H, W), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += q[dy:dy + H, dx:dx + W]
    return out


def sums(img, r):
    """(a, b, c) as int64 H x W."""
    kx, ky = differences(img)
    return window_sum(kx * kx, r), window_sum(kx * ky, r), window_sum(ky * ky, r)


def score_of_sums(a, b, c, r, with_d=False):
    """The double part of the definition on integer sums: float32 scores (and the unclamped d)."""
    n = (2 * r + 1) ** 2
    a, b, c = (np.asarray(v, np.int64) for v in (a, b, c))
    tr = (a + c).astype(np.float64)
    dac, db = (a - c).astype(np.float64), b.astype(np.float64)
    s = np.sqrt(dac * dac + 4.0 * db * db)
    d = tr - s
    sc = np.sqrt(np.where(d < 0, 0.0, d) / (8.0 * n)).astype(np.float32)
    return (sc, d) if with_d else sc


def score(img, r):
    """The H x W float32 score image."""
    assert r in (1, 2, 3)
    return score_of_sums(*sums(img, r), r)


@contextlib.contextmanager
def swapped_response(r):
    """Inside: the host detector of the pairs tests (grid selection, every candidate, host_levels) reads the corner score of
    radius r where it read the gradient magnitude.  r None or 0: nothing is swapped."""
    old = pairs_ref.gradient_magnitude
    if r:
        pairs_ref.gradient_magnitude = lambda img: score(img, r)
    try:
        yield
    finally:
        pairs_ref.gradient_magnitude = old


def keypoints(img, level, H0, W0, cell, thr, depth, border, r, dense):
    """(xy K x 2, z K) of one level under the corner score (r = 0: under the gradient magnitude)."""
    import pairs_dense_ref as dref
    with swapped_response(r):
        if dense:
            return dref.keypoints(img, level, thr, depth, border)
        return pairs_ref.keypoints(img, level, H0, W0, cell, cell, thr, depth, border)


@contextlib.contextmanager
def scored_object(name, r, thr):
    """Inside: pairs_oracle.host_levels(name) -- also where tests/pairs_entries_support.py calls it -- restates the option-laden
    object `name` with a detector that reads the corner score of radius r above thr (the caller's points of object D have no
    detector: unchanged)."""
    import pairs_oracle as po
    saved = po.OBJECTS[name]
    po.OBJECTS[name] = dict(saved, thr=thr)
    try:
        with swapped_response(r):
            yield
    finally:
        po.OBJECTS[name] = saved


def host_levels(name, r, thr, c=None):
    import pairs_oracle as po
    with scored_object(name, r, thr):
        return po.host_levels(name, c)


# ---------------------------------------------------------------------------------------------------------------- test images
def checkerboard(H, W):
    """0 / 255 in squares of two pixels: right and left (bottom and top) always lie in different squares, so |kx| = |ky| = 255 at
    every interior pixel (squares of one pixel would have no central differences at all)."""
    y, x = np.mgrid[0:H, 0:W]
    return (255 * ((((x >> 1) + (y >> 1)) & 1))).astype(np.uint8)


def images(H, W, seed):
    """The contents of the device tests: random bytes, a constant, a vertical step, a diagonal step, the 0/255 checkerboard."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return dict(random=rng.integers(0, 256, (H, W)).astype(np.uint8), constant=np.full((H, W), 77, np.uint8),
                vstep=np.where(x >= W // 2, 200, 30).astype(np.uint8), dstep=np.where(x + y >= (H + W) // 2, 220, 15).astype(np.uint8),
                checker=checkerboard(H, W))
