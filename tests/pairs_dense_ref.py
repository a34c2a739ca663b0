"""numpy restatement of what one (pair, level) of a batch prepared with mbavo_pairs_opts.every_candidate = 1 must hold: every
pixel of the keyframe level whose gradient magnitude exceeds the threshold (FeatureDetectorSemiDense.cpp:27-43, no
FeatureDetectorBase::gridSelection), whose depth at its level-0 position is not below 1e-2 (blur_aware_direct_tracker.cpp:389-415)
and which lies inside the border margin, in row-major order.  tests/test_pairs_dense_api.py pins it to the oracle's detector on
the CPU; tests/test_gpu_pairs_dense.py holds the device against it."""
import numpy as np

import pairs_ref


def candidates(img, thr):
    """(x, y) int arrays of the pixels with gradient magnitude > thr, row-major."""
    ys, xs = np.nonzero(pairs_ref.gradient_magnitude(img) > np.float32(thr))  # (np.nonzero walks C order: rows, then columns)
    return xs, ys


def depths(xs, ys, level, depth):
    """The float32 depths at the level-0 positions int(x * 2^level + 0.5), as float64."""
    s = 2.0 ** level
    x0 = (xs.astype(np.float32) * s + 0.5).astype(np.int64)
    y0 = (ys.astype(np.float32) * s + 0.5).astype(np.int64)
    return depth[y0, x0].astype(np.float64)


def keypoints(img, level, thr, depth, border):
    """(xy K x 2 float64, z K float64) of one level."""
    H, W = img.shape
    xs, ys = candidates(img, thr)
    z = depths(xs, ys, level, depth)
    ok = ~(z < 1e-2)
    xy = np.stack([xs[ok], ys[ok]], 1).astype(np.float64).reshape(-1, 2)
    return pairs_ref.border_filter(xy, z[ok], H, W, border)


def capacities(H0, W0, L):
    return [(H0 >> l) * (W0 >> l) for l in range(L)]


def ramp(H, W):
    """(c + r) % 251: every interior pixel has a gradient (|dx| or |dy| >= 0.5 ... 125), so with depth 1 and border 0 every
    interior pixel is a keypoint: K = (H - 2)(W - 2), the largest a level can have."""
    r, c = np.mgrid[0:H, 0:W]
    return ((c + r) % 251).astype(np.uint8)
