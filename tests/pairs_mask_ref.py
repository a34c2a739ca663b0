"""numpy restatement of the caller-supplied masks of include/mbavo.h (mbavo_pairs_opts.mask, mbavo_pairs_set_masks,
mbavo_undistort_mask_batch, mbavo_mask_clearance_batch): the warp of a raw-geometry mask, once as loops that read like the
definition and once vectorised, and "valid at level 0 with a mask".  Everything above level 0 -- "valid at level l", "clear at
radius r" -- is tests/pairs_valid_ref.py's, unchanged.  tests/test_pairs_mask_api.py holds the two forms to each other on the CPU;
tests/test_gpu_pairs_mask.py holds the device to them byte for byte.  Integer and comparison logic: exact.

It also makes the masks the tests use, for the 60 x 80 raw camera of pairs_valid_ref: a bonnet, a scatter of single masked raw
pixels, and masks planted around the whole-coordinate and limit entries of pairs_valid_ref.handcrafted_map()."""
import math

import numpy as np

import pairs_valid_ref as vref

HS, WS = vref.HS, vref.WS


# ---- the definition, as loops
def warp_mask_loops(raw, map_xy):
    """H x W uint8 of 0 / 1: the entry valid by the level-0 rule and `raw` non-zero at every tap that carries weight."""
    Hs, Ws = raw.shape
    h, w = map_xy.shape[:2]
    out = np.zeros((h, w), np.uint8)
    for r in range(h):
        for c in range(w):
            X, Y = float(map_xy[r, c, 0]), float(map_xy[r, c, 1])  # (float32 -> double: exact)
            if not (0.0 <= X and X <= float(Ws - 1) and 0.0 <= Y and Y <= float(Hs - 1)):
                continue  # (NaN and +-inf fail the comparisons)
            x0, y0 = int(math.floor(X)), int(math.floor(Y))
            ax, ay = X - math.floor(X), Y - math.floor(Y)
            taps = [(x0, y0)]
            if ax > 0:
                taps.append((x0 + 1, y0))
            if ay > 0:
                taps.append((x0, y0 + 1))
            if ax > 0 and ay > 0:
                taps.append((x0 + 1, y0 + 1))
            ok = True
            for tx, ty in taps:
                assert 0 <= tx < Ws and 0 <= ty < Hs  # (a valid entry reads no tap outside the raw image)
                ok = ok and raw[ty, tx] != 0
            out[r, c] = 1 if ok else 0
    return out


# ---- the same, vectorised
def warp_mask(raw, map_xy):
    Hs, Ws = raw.shape
    v = vref.valid0(map_xy, Hs, Ws)
    X, Y = (np.where(v, map_xy[..., i].astype(np.float64), 0.0) for i in (0, 1))
    fx, fy = np.floor(X), np.floor(Y)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    right, below = (X - fx) > 0, (Y - fy) > 0
    x1, y1 = np.where(right, x0 + 1, x0), np.where(below, y0 + 1, y0)  # (a tap without weight: the tap beside it again)
    assert x1.max() < Ws and y1.max() < Hs
    usable = raw != 0
    return (v & usable[y0, x0] & usable[y0, x1] & usable[y1, x0] & usable[y1, x1]).astype(np.uint8)


def valid0(map_xy, mask, Hs=HS, Ws=WS):
    """H x W bool, "valid at level 0 with a mask": the map term (true where there is no map: map_xy None) and mask != 0 (true
    where there is no mask: None)."""
    assert map_xy is not None or mask is not None
    v = vref.valid0(map_xy, Hs, Ws) if map_xy is not None else np.ones(mask.shape, bool)
    return v if mask is None else v & (mask != 0)


def clearance(map_xy, mask, levels, r, Hs=HS, Ws=WS):
    """[level 0, .., level levels-1] uint8 of the map (or None) and the undistorted-geometry mask (or None)."""
    return vref.clearance(valid0(map_xy, mask, Hs, Ws), levels, r)


# ---- the test masks (usable bytes are not all 1: any byte != 0 counts)
def bonnet(Hs=HS, Ws=WS, height=0.45, half_width=0.62):
    """A vehicle bonnet: a half-ellipse at the bottom of the raw image, centred a little off the middle; 0 inside, 255 outside."""
    y, x = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    inside = ((x - (0.5 * Ws + 1.5)) / (half_width * Ws)) ** 2 + ((Hs - 1 - y) / (height * Hs)) ** 2 <= 1.0
    return np.where(inside, 0, 255).astype(np.uint8)


def scatter(Hs=HS, Ws=WS, seed=5, share=0.04):
    """Single masked raw pixels; the usable bytes take every value 1 .. 255."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 256, (Hs, Ws)).astype(np.uint8)
    m[rng.uniform(0, 1, (Hs, Ws)) < share] = 0
    return m


def bonnet_undistorted(h=vref.H, w=vref.W):
    """The same shape drawn directly in an h x w undistorted image (for objects without a map)."""
    return bonnet(h, w)


def planted(Hs=HS, Ws=WS):
    """A raw mask for pairs_valid_ref.handcrafted_map(): usable everywhere but next to the raw pixels its whole-coordinate and limit
    entries point at.  The plain entries of that map sit at (Ws / 2, Hs / 2) = (40, 30), a whole coordinate: its right, lower and
    diagonal neighbours are masked (taps of weight 0), and so are the neighbours of the entries at (0, 0), (1, 0..), and the raw
    pixels two steps inside the limits, which the nextafter entries reach with a tiny weight."""
    m = np.full((Hs, Ws), 200, np.uint8)
    for x, y in ((Ws // 2 + 1, Hs // 2), (Ws // 2, Hs // 2 + 1), (Ws // 2 + 1, Hs // 2 + 1),  # around the plain entry
                 (1, 0), (0, 1), (1, 1),                                                   # around (0, 0) and (-0.0, -0.0)
                 (Ws - 2, 1), (Ws - 2, 2),                                                 # what down(Ws - 1) reaches: (Ws - 2, 1)
                 (2, Hs - 2), (1, Hs - 2),                                                 # what down(Hs - 1) reaches: (1, Hs - 2)
                 (2, 1), (1, 2), (2, 2)):                                                  # right of / below up(0) entries at (0+, 1), (1, 0+)
        m[y, x] = 0
    return m


MASKS = {"bonnet": bonnet, "scatter": scatter, "planted": planted}
