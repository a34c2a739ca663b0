"""Inputs that more than one pairs test file uses, each made once per session and left unchanged: the base images and depth maps,
raw depth maps with holes, the radial-tangential undistortion cases (which the unified-model and the camera-set tests share
their raw images and helpers with) and the clearance-mask case."""
import numpy as np

import pairs_dense_ref as dref
import pairs_depth_ref as zref
import pairs_ref
import pairs_undistort_ref as uref
import pairs_valid_ref as vref
from mba_vo_amd import synth


def inputs(B, H, W, seed=1, special=True):
    """Distinct images and depth maps per pair; depth maps with holes (0 and a positive value below 1e-2).  With `special` and
    B >= 3: pair 1 is a constant image, pair 2 a flat image with two equal maxima in one grid cell."""
    rng = np.random.default_rng(seed)
    base = synth.texture_image(H, W, seed=seed, octaves=(32, 16, 8, 4))
    other = synth.texture_image(H, W, seed=seed + 100, octaves=(32, 16, 8, 4))
    sharp = np.stack([np.roll(base, (7 * b, 13 * b), (0, 1)) for b in range(B)])
    blur = np.stack([np.roll(other, (3 * b + 1, 5 * b + 2), (0, 1)) for b in range(B)])
    depth = rng.uniform(0.5, 3.0, (B, H, W)).astype(np.float32)
    holes = rng.uniform(0, 1, (B, H, W))
    depth[holes < 0.15] = 0.0
    depth[(holes >= 0.15) & (holes < 0.2)] = 0.005
    if special and B >= 3:
        sharp[1] = 93
        sharp[2] = 100
        sharp[2, 45, 46] = sharp[2, 47, 43] = 160  # equal magnitudes at their neighbours, all inside one level-0 cell
        depth[2] = 1.5
    return np.ascontiguousarray(sharp), depth, np.ascontiguousarray(blur)


def borders(L, on):
    return [max(4, 20 >> l) if on else 0 for l in range(L)]


def raw_depth(fmt, B, H, W, seed, beyond=None):
    """B raw maps in depth format fmt with holes (0 and a value below 1e-2); `beyond`: a distance planted in a further 4 %."""
    rng = np.random.default_rng(seed)
    holes = rng.uniform(0, 1, (B, H, W))
    if fmt == 2:
        raw = rng.integers(2500, 15000, (B, H, W)).astype(np.uint16)  # 0.5 .. 3 m
        raw[holes < 0.12], raw[(holes >= 0.12) & (holes < 0.17)] = 0, 25
    else:
        raw = rng.uniform(0.5, 3.0, (B, H, W)).astype(np.float32)
        raw[holes < 0.12], raw[(holes >= 0.12) & (holes < 0.17)] = 0.0, 0.005
    if beyond is not None:
        raw[(holes >= 0.17) & (holes < 0.21)] = beyond
    return raw


# ---- undistortion: 48 x 64 from a 52 x 76 raw camera, 50 x 70 from 50 x 70; B = 3, L = 3
CELL, THR, BORDERS = 6, 3.0, (3, 2, 1)  # small cells and margins: every level of a 48 x 64 pyramid keeps keypoints
DISTS = {"outside": uref.DIST_OUTSIDE, "inside": uref.DIST_INSIDE, "none": uref.DIST_NONE}
DEPTH_FORMATS = {0: dict(depth_format=0, depth_unit=0.0, depth_max=0.0), 1: zref.UNREAL, 2: zref.ETH3D}


def _undistort_geometry(shape):
    """(H, W, Hs, Ws, to_intr, from_intr): the undistorted camera and the raw one."""
    if shape in ("crop", "wide"):  # a 52 x 76 sensor undistorted into 48 x 64
        H, W, Hs, Ws = 48, 64, 52, 76
        K = uref.intrinsics(H, W)
        if shape == "wide":  # the tests' camera at the raw size: the first coefficient set reaches three rows past the raw image
            return H, W, Hs, Ws, K, uref.intrinsics(Hs, Ws)
        # a shorter vertical focal length: the first set still points outside, the second stays inside
        return H, W, Hs, Ws, K, (517.3 * Ws / 640, 1.12 * K[1], (Ws - 1) / 2 + 0.3, (Hs - 1) / 2 - 0.2)
    H, W = 50, 70  # the same camera and size on both sides
    return H, W, H, W, uref.intrinsics(H, W), uref.intrinsics(H, W)


_UNDISTORT = {}


def undistort_case(shape, dist):
    """Everything numpy of one (shape, coefficient set), made once: the map, raw images and depth maps of B = 3 pairs (and a
    second set for an update), their remapped versions."""
    key = (shape, dist)
    if key not in _UNDISTORT:
        H, W, Hs, Ws, to_intr, from_intr = _undistort_geometry(shape)
        B = 3
        m = uref.undistort_map(from_intr, DISTS[dist], to_intr, H, W)
        tex = lambda seed: np.stack([synth.texture_image(Hs, Ws, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        raw = dict(sharp=tex(7), blur=tex(107), new_sharp=tex(40), new_blur=tex(140))
        und = {k: np.stack([uref.remap_u8(im, m) for im in v]) for k, v in raw.items()}
        rng = np.random.default_rng(5)
        z = rng.uniform(0.5, 3.0, (2, B, H, W)).astype(np.float32)  # depth in the undistorted geometry, with holes
        z[rng.uniform(0, 1, z.shape) < 0.15] = 0.0
        _UNDISTORT[key] = dict(shape=shape, dist=dist, H=H, W=W, Hs=Hs, Ws=Ws, L=3, B=B, intr=to_intr, from_intr=from_intr, map=m, raw=raw, und=und,
                               z=z[0], new_z=z[1], outside=uref.tap_outside(m, Hs, Ws))
    return _UNDISTORT[key]


def witness(c):
    """What the coefficient set is there for."""
    share = float(c["outside"].mean())
    if c["dist"] == "outside":
        assert 0.01 < share < 0.10, share
    elif c["dist"] == "inside":
        assert share == 0.0
    return share


def undistort_camera(c, dist=None):
    from mba_vo_amd import workloads
    return workloads.camera_radtan(c["Hs"], c["Ws"], c["from_intr"], DISTS[dist or c["dist"]])


def undistort_batch(ctx, c, undistort, dense=False, kf=0, depth=0, B=None, L=None, borders=BORDERS, **kw):
    from mba_vo_amd import workloads
    L = L or c["L"]
    return workloads.PairBatch(ctx, B or c["B"], L=L, H=c["H"], W=c["W"], intr=c["intr"], border=list(borders[:L]), cell=0 if dense else CELL, thresh=THR,
                               every_candidate=dense, keyframe_format=kf, undistort=undistort, **dict(DEPTH_FORMATS[depth], **kw))


def restated(c, got, z_of_pair, dense, borders):
    """Per (pair, level) the numpy keypoints (xy, z) on the device's own image levels and the numpy z maps."""
    out = []
    for e, g in enumerate(got):
        b, l = divmod(e, c["L"])
        im = g["ref"].reshape(c["H"] >> l, c["W"] >> l)
        out.append(dref.keypoints(im, l, THR, z_of_pair[b], borders[l]) if dense else
                   pairs_ref.keypoints(im, l, c["H"], c["W"], CELL, CELL, THR, z_of_pair[b], borders[l]))
    return out


def special_map(c):
    """The case's map with the entries the remap's rules are about planted in it."""
    m = c["map"].copy()
    Hs, Ws = c["Hs"], c["Ws"]
    planted = [(np.nan, 3.0), (3.0, np.nan), (np.inf, 1.0), (2.0 ** 31, 5.0), (5.0, -2.0 ** 31), (2.0 ** 30, 1.0), (-0.5, 4.0), (Ws - 0.5, 4.0),
               (4.0, Hs - 1.0), (4.25, Hs - 0.5), (-1.0, 2.0), (Ws - 1.0, Hs - 1.0), (-0.25, -0.25), (float(Ws), 3.0), (7.5, 9.5)]
    flat = m.reshape(-1, 2)
    at = np.linspace(0, flat.shape[0] - 1, len(planted)).astype(int)  # the first and the last pixel among them
    flat[at] = np.array(planted, np.float32)
    return m


# ---- the clearance mask: pairs_valid_ref's two cameras and sizes, B = 3
VALID_B, VALID_NAMES = 3, ("radtan", "unified")
_VALID = {}


def valid_case():
    """Everything numpy, made once and left unchanged: the maps and their level-0 validity, raw images (two sets) and depth maps
    in the undistorted geometry (float z) and in the raw one (uint16)."""
    if not _VALID:
        tex = lambda seed: np.stack([synth.texture_image(vref.HS, vref.WS, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(VALID_B)])
        maps = {n: vref.camera_map(vref.CAMERAS[n]) for n in VALID_NAMES}
        _VALID.update(maps=maps, valid0={n: vref.valid0(m, vref.HS, vref.WS) for n, m in maps.items()},
                      sharp=tex(7), blur=tex(107), new_sharp=tex(40), new_blur=tex(140),
                      depth={0: raw_depth(0, VALID_B, vref.H, vref.W, seed=31), 2: raw_depth(2, VALID_B, vref.HS, vref.WS, seed=40)},
                      new_depth={0: raw_depth(0, VALID_B, vref.H, vref.W, seed=81), 2: raw_depth(2, VALID_B, vref.HS, vref.WS, seed=90)})
    return _VALID


def valid_camera(name):
    from mba_vo_amd import workloads
    cam = vref.CAMERAS[name]
    if cam["model"] == 2:
        return workloads.camera_unified(vref.HS, vref.WS, cam["from_intr"], cam["xi"], cam["dist"])
    return workloads.camera_radtan(vref.HS, vref.WS, cam["from_intr"], cam["dist"])


def valid_device_map(ctx, name):
    from mba_vo_amd import workloads
    cam = vref.CAMERAS[name]
    return workloads.undistort_map(ctx, valid_camera(name), cam["to_intr"], vref.H, vref.W)


def filtered(entries, clear_of_pair):
    """The keypoint lists of an unmasked object, every (pair, level) filtered by its clearance, in order; (dropped, kept) at level 0."""
    out, dropped, kept = [], 0, 0
    for e, g in enumerate(entries):
        b, l = divmod(e, vref.L)
        xy = g["xy"]
        x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
        assert np.array_equal(x, xy[:, 0]) and np.array_equal(y, xy[:, 1])
        keep = clear_of_pair[b][l][y, x] == 1
        out.append(dict(g, xy=np.ascontiguousarray(xy[keep]), z=np.ascontiguousarray(g["z"][keep])))
        if l == 0:
            dropped, kept = dropped + int((~keep).sum()), kept + int(keep.sum())
    return out, dropped, kept


def counts_of(entries):
    return np.array([len(g["z"]) for g in entries], np.int32).reshape(-1, vref.L)
