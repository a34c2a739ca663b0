"""numpy restatement of what one (pair, level) of a prepared batch must hold: grid geometry (FeatureDetectorBase.cpp:56-64),
semi-dense candidates and grid selection (FeatureDetectorSemiDense.cpp:27-43, FeatureDetectorBase.cpp:49-91), depth lookup
(blur_aware_direct_tracker.cpp:389-415), border filter and ordered compaction.  tests/test_pairs_api.py pins it to the oracle's
detector on the CPU; tests/test_gpu_pairs_prep.py holds the device against it."""
import numpy as np


def grid(H0, W0, level, cell_H, cell_W):
    """(cell height, cell width, cell rows, cell columns) of a pyramid level."""
    ch, cw = int(cell_H / 1.414 ** level), int(cell_W / 1.414 ** level)
    sf = int(2 ** level)
    return ch, cw, (H0 // sf) // ch + 1, (W0 // sf) // cw + 1


def cells_per_level(H0, W0, L, cell_H, cell_W):
    return [g[2] * g[3] for g in (grid(H0, W0, l, cell_H, cell_W) for l in range(L))]


def gradient_magnitude(img):
    """Gradient.h:56-71 in float32; zero on the 1-pixel border."""
    f = img.astype(np.float32)
    dx, dy = np.zeros_like(f), np.zeros_like(f)
    dx[1:-1, 1:-1] = np.float32(0.5) * (f[1:-1, 2:] - f[1:-1, :-2])
    dy[1:-1, 1:-1] = np.float32(0.5) * (f[2:, 1:-1] - f[:-2, 1:-1])
    return np.sqrt(dx * dx + dy * dy)


def picks(mag, level, H0, W0, cell_H, cell_W, thr):
    """Per grid cell, in row-major cell order: (x, y) of the first pixel (row-major) of strictly largest magnitude among those
    above the threshold, or None."""
    H, W = mag.shape
    ch, cw, nch, ncw = grid(H0, W0, level, cell_H, cell_W)
    assert (H - 1) // ch < nch and (W - 1) // cw < ncw
    m = np.zeros((nch * ch, ncw * cw), np.float32)
    m[:H, :W] = np.where(mag > np.float32(thr), mag, np.float32(0))
    c = m.reshape(nch, ch, ncw, cw).transpose(0, 2, 1, 3).reshape(nch * ncw, ch * cw)
    arg = c.argmax(1)  # the first of equal maxima: lower (row, column) within the cell = lower row-major index
    best = c[np.arange(c.shape[0]), arg]
    out = []
    for ci in range(nch * ncw):
        if best[ci] > 0 and not best[ci] < 1e-6:
            out.append(((ci % ncw) * cw + int(arg[ci]) % cw, (ci // ncw) * ch + int(arg[ci]) // cw))
        else:
            out.append(None)
    return out


def keypoints(img, level, H0, W0, cell_H, cell_W, thr, depth, border):
    """(xy K x 2 float64, z K float64): the kept picks in cell order -- depth at the level-0 position not below 1e-2, inside the
    border margin."""
    H, W = img.shape
    xy, zs = [], []
    for p in picks(gradient_magnitude(img), level, H0, W0, cell_H, cell_W, thr):
        if p is None:
            continue
        x, y = p
        z = depth[int(np.float32(y) * 2.0 ** level + 0.5), int(np.float32(x) * 2.0 ** level + 0.5)]
        if float(z) < 1e-2:
            continue
        if not (border <= x < W - border and border <= y < H - border):
            continue
        xy.append((x, y))
        zs.append(float(z))
    return np.array(xy, np.float64).reshape(-1, 2), np.array(zs, np.float64)


def border_filter(xy, z, H, W, m):
    """The filter RenderedPairPyramids applies behind mbavo_detect_semidense, order kept."""
    ok = (xy[:, 0] >= m) & (xy[:, 0] < W - m) & (xy[:, 1] >= m) & (xy[:, 1] < H - m)
    return xy[ok], z[ok]


def oracle_keypoints(orc, im, lv, H0, W0, cell, thr, depth, border):
    """The oracle's detector and depth lookup on one level, then the border filter in its order: ((xy, z), magnitude image)."""
    L = orc.lib()
    H, W = im.shape
    im = np.ascontiguousarray(im)
    g, mag = np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.float32)
    L.orc_image_gradients_u8(orc.u8p(im), H, W, orc.fp(g), orc.fp(mag))
    xy = np.zeros(2 * H * W, np.float32)
    n = L.orc_detect_semidense(orc.fp(mag), H, W, lv, H0, W0, cell, cell, thr, orc.fp(xy), None, H * W)
    oxy, oz = np.zeros(2 * max(n, 1)), np.zeros(max(n, 1))
    K = L.orc_keypoint_depths(orc.fp(xy), n, lv, orc.fp(np.ascontiguousarray(depth)), H0, W0, orc.dp(oxy), orc.dp(oz)) if n else 0
    return border_filter(oxy[:2 * K].reshape(-1, 2), oz[:K], H, W, border), mag
