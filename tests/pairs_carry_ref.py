"""numpy restatement of mbavo_pairs_carry_save and mbavo_pairs_carry_adopt (include/mbavo.h) on one (pair, level) (helper, no test in
it): brute force -- no bins, no index, every new keypoint against every carried point -- and the sums of the adopt formed keypoint by
keypoint over ascending source index, each product rounded, added left to right.  float64, operation by operation as the header
writes them.  The records' sums are formed as the header says the device forms them (`record_sum`)."""
import ctypes as C

import numpy as np

EMPTY, ADOPTED, SPARSE, RANGE = 0, 1, 2, 3
_QUIET = dict(divide="ignore", invalid="ignore", over="ignore")


def rotation(q):
    """R of a unit quaternion (x, y, z, w), row-major, in the header's term order."""
    x, y, z, w = (np.float64(v) for v in q)
    return np.array([[w * w + x * x - y * y - z * z, -2.0 * (w * z - x * y), 2.0 * (w * y + x * z)],
                     [2.0 * (w * z + x * y), w * w - x * x + y * y - z * z, -2.0 * (w * x - y * z)],
                     [-2.0 * (w * y - x * z), 2.0 * (w * x + y * z), w * w - x * x - y * y + z * z]])


def level_intrinsics(intr, l):
    return tuple(np.float64(v) / np.float64(1 << l) for v in intr)


def record_sum(terms, cap):
    """A record's sum over per-keypoint terms (0.0 where a keypoint adds nothing): keypoint i in lane i mod 256 of workgroup
    (i / 256) mod G, a lane's keypoints ascending; a butterfly over the 64 lanes of a wave, the four waves in order, the G workgroups
    from 0.0 in order."""
    terms = np.asarray(terms, np.float64)
    K = terms.size
    G = min(64, max(1, (cap + 255) // 256))
    acc = np.zeros((G, 256))
    for t in range((K + 255) // 256):
        part = terms[256 * t:256 * t + 256]
        acc[t % G, :part.size] = acc[t % G, :part.size] + part
    idx = np.arange(64)
    blocks = []
    for g in range(G):
        v = acc[g].reshape(4, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, idx ^ off]
        blocks.append(((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])
    if G == 1:
        return float(blocks[0])
    r = np.float64(0.0)
    for b in blocks:
        r = r + b
    return float(r)


def save(xy, z, intr, W, H, T, deflate=1.0, w=None, z_min=0.0, z_max=0.0, cap=None):
    """The save on one (pair, level): xy K x 2 and z the old keyframe's keypoints at that level, intr the level's (fx, fy, cx, cy), T
    = (t, q xyzw) with X_old = R X_new + t, w None (ones) or the filter's info per keypoint.  Returns dict(carried K bools, px K x 2
    ints, rho, w (meaningful where carried), D_new, and the record's fields); cap: the level's keypoint capacity (the sums' grid)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z = np.asarray(z, np.float64)
    K = z.size
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    t, R = np.asarray(T[:3], np.float64), rotation(T[3:7])
    z_min = 1e-2 if z_min == 0 else z_min
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    with np.errstate(**_QUIET):
        valid = np.isfinite(z) & (z > 0)
        rx, ry = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
        d0, d1, d2 = z * rx - t[0], z * ry - t[1], z - t[2]
        X = (R[0, 0] * d0 + R[1, 0] * d1) + R[2, 0] * d2
        Y = (R[0, 1] * d0 + R[1, 1] * d1) + R[2, 1] * d2
        Dn = (R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2
        ok = valid & np.isfinite(Dn) & (Dn >= z_min) & ((z_max == 0) | (Dn <= z_max))
        u, v = fx * (X / Dn) + cx, fy * (Y / Dn) + cy
        xf, yf = np.floor(u + 0.5), np.floor(v + 0.5)
        ok &= (xf >= 0) & (xf < W) & (yf >= 0) & (yf < H)
        c = (R[0, 2] * rx + R[1, 2] * ry) + R[2, 2]
        s = (c * (z * z)) / (Dn * Dn)
        wn = (w / (s * s)) * np.float64(deflate)
        ok &= (wn > 0) & np.isfinite(wn)
        rho = 1.0 / Dn
    px = np.stack([np.where(ok, xf, -1), np.where(ok, yf, -1)], 1).astype(np.int64)
    cap = max(K, 1) if cap is None else cap
    return dict(carried=ok, px=px, rho=np.where(ok, rho, 0.0), w=np.where(ok, wn, 0.0), D_new=Dn, num_keypoints=K, num_valid=int(valid.sum()),
                num_carried=int(ok.sum()), sum_w=record_sum(np.where(ok, wn, 0.0), cap))


def adopt(xy, z, carried, radius, min_support=1, max_rel_diff=0.1, z_min=0.0, z_max=0.0, prior_rel_sigma=0.0, max_info=0.0, cap=None,
          order=None):
    """The adopt on one (pair, level): xy K x 2 and z the NEW keyframe's keypoints as the update left them, `carried` what `save`
    returned for that (pair, level).  `order`: None, or a function that reorders a keypoint's ascending foreground list before the
    sums.  Returns dict(rho, info, count, flags, z_new (the depths after apply = 1), mu, info_state (the filter's state after
    seed_filter = 1), and the record's fields)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z = np.asarray(z, np.float64)
    K = z.size
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    js = np.flatnonzero(carried["carried"])  # ascending source index
    cx, cy, crho, cw = carried["px"][js, 0], carried["px"][js, 1], carried["rho"][js], carried["w"][js]
    z_min = 1e-2 if z_min == 0 else z_min
    rho, info = np.full(K, np.nan), np.zeros(K)
    count, flags = np.zeros(K, np.int32), np.zeros(K, np.uint8)
    z_new = z.copy()
    rel2 = np.zeros(K)
    with np.errstate(**_QUIET):
        mu = 1.0 / z
        prs = np.float64(prior_rel_sigma)
        info_state = np.zeros(K) if prior_rel_sigma == 0 else 1.0 / ((prs * mu) * (prs * mu))
        for i in range(K):
            near = (np.abs(cx - x[i]) <= radius) & (np.abs(cy - y[i]) <= radius)
            if not near.any():
                continue
            rho_max = crho[near].max()
            fg = np.flatnonzero(near & (crho >= (np.float64(1.0) - np.float64(max_rel_diff)) * rho_max))
            if order is not None:
                fg = order(fg)
            count[i] = fg.size
            flags[i] = SPARSE
            if fg.size < min_support:
                continue
            SW, SR = np.float64(0.0), np.float64(0.0)
            for j in fg:
                SW = SW + cw[j]
                SR = SR + cw[j] * crho[j]
            rho_n = SR / SW
            D = np.float64(1.0) / rho_n
            if not (np.isfinite(D) and D >= z_min and (z_max == 0 or D <= z_max)):
                flags[i] = RANGE
                continue
            flags[i], rho[i], info[i], z_new[i] = ADOPTED, rho_n, SW, D
            mu[i], info_state[i] = rho_n, (SW if (max_info == 0 or SW <= max_info) else max_info)
            if np.isfinite(z[i]) and z[i] > 0:
                ri = np.float64(1.0) / z[i]
                rel = (rho_n - ri) / ri
                rel2[i] = rel * rel
    cap = max(K, 1) if cap is None else cap
    return dict(rho=rho, info=info, count=count, flags=flags, z_new=z_new, mu=mu, info_state=info_state, num_keypoints=K,
                num_adopted=int((flags == ADOPTED).sum()), num_empty=int((flags == EMPTY).sum()), sum_info=record_sum(info, cap),
                sum_sq_rel=record_sum(rel2, cap))


def relative_pose(pa, qa, pb, qb):
    """T = (t, q) of camera B in camera A's frame, X_A = R X_B + t, from the two cameras' world poses (p, q xyzw; X_w = R(q) X_c +
    p)."""
    Ra, Rb = rotation(qa), rotation(qb)
    t = Ra.T @ (np.asarray(pb, np.float64) - np.asarray(pa, np.float64))
    qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    ax, ay, az, aw = -qa[0], -qa[1], -qa[2], qa[3]
    bx, by, bz, bw = qb
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz])
    assert np.allclose(rotation(q), Ra.T @ Rb, atol=1e-12)
    return np.concatenate([t, q / np.linalg.norm(q)])


def save_opts(capi, radius=2, deflate=1.0, weights=0, z_min=0.0, z_max=0.0):
    o = capi.PairsCarrySaveOpts()
    o.weights, o.radius, o.deflate, o.z_min, o.z_max = weights, radius, deflate, z_min, z_max
    return o


def adopt_opts(capi, min_support=1, max_rel_diff=0.1, apply=0, seed_filter=0, z_min=0.0, z_max=0.0, prior_rel_sigma=0.0, max_info=0.0):
    o = capi.PairsCarryAdoptOpts()
    o.apply, o.seed_filter, o.min_support = apply, seed_filter, min_support
    o.max_rel_diff, o.z_min, o.z_max, o.prior_rel_sigma, o.max_info = max_rel_diff, z_min, z_max, prior_rel_sigma, max_info
    return o


def call_save(lib, handle, pairs, T, o, out=None):
    """The raw entry point with optional ctypes records; pairs / T: numpy arrays or None."""
    n = 0 if pairs is None else len(pairs)
    ip = None if pairs is None else np.ascontiguousarray(pairs, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = None if T is None else np.ascontiguousarray(T, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    return lib.mbavo_pairs_carry_save(handle, n, ip, dp, None if o is None else C.byref(o), out)


def call_adopt(lib, handle, pairs, o, out=None):
    n = 0 if pairs is None else len(pairs)
    ip = None if pairs is None else np.ascontiguousarray(pairs, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    return lib.mbavo_pairs_carry_adopt(handle, n, ip, None if o is None else C.byref(o), out, None, None, None, None)


# ---- the property's setting (tests/test_pairs_carry_api.py says where it comes from): two keyframes of a RenderedScene-like plane
PROPERTY = dict(radius=2, min_support=1, max_rel_diff=0.1)


def plane_depth(xy, intr, p, q, D):
    """z-depth, in the camera with world pose (p, q), of the plane z = D (world) along the rays of the pixels xy (the formula of
    workloads.RenderedScene.render)."""
    R = rotation(q)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    rz = (xy[:, 0] - intr[2]) / intr[0] * R[2, 0] + (xy[:, 1] - intr[3]) / intr[1] * R[2, 1] + R[2, 2]
    return (D - p[2]) / rz


def plane_gradient(xy, intr, p, q, D):
    """The analytic relative depth change of that plane in that camera over one pixel, per pixel of xy: |d log depth / dx| + |d log
    depth / dy|, the most a step of one pixel in both axes can change it."""
    R = rotation(q)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    rz = (xy[:, 0] - intr[2]) / intr[0] * R[2, 0] + (xy[:, 1] - intr[3]) / intr[1] * R[2, 1] + R[2, 2]
    return np.abs(R[2, 0] / intr[0] / rz) + np.abs(R[2, 1] / intr[1] / rz)


def property_scene(lib, capi, H=48, W=64, wrong=5.0):
    """Two keyframes of a workloads.RenderedScene (frames 0 and 3 of its world spline, no GPU): keyframe A's keypoints on a grid of
    pitch 2 with the plane's exact depths, keyframe B's on the odd grid at the constant depth `wrong`, T from the scene's true poses.
    Returns dict(intr, T, A=(xy, z), B=(xy, z), truth (the plane's depth at B's keypoints), grad (plane_gradient at them), shift (the
    largest displacement, in pixels, of a plane point between the two keyframes))."""
    from mba_vo_amd import workloads
    sc = workloads.RenderedScene(None, 4, H, W, "cpu", 3, 7.5, 0.1, 0.04, 0.0)
    poses = []
    for b in (0, 3):
        p, q = np.zeros(3), np.zeros(4)
        assert lib.mbavo_spline_get_pose(4, sc.t0w, sc.dtk, capi.dp(sc.ktw), capi.dp(sc.kRw), sc.n_world, float(sc.times(b)[0]), capi.dp(p), capi.dp(q),
                                         None, None) == 0
        poses.append((p, q / np.linalg.norm(q)))
    (pa, qa), (pb, qb) = poses
    T = relative_pose(pa, qa, pb, qb)
    ys, xs = np.meshgrid(np.arange(0, H, 2), np.arange(0, W, 2), indexing="ij")
    xa = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    ys, xs = np.meshgrid(np.arange(1, H, 2), np.arange(1, W, 2), indexing="ij")
    xb = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    za = plane_depth(xa, sc.intr, pa, qa, sc.D)
    # where A's plane points fall in B, by matrices (the test's own geometry, not the restatement's)
    Xa = np.stack([(xa[:, 0] - sc.intr[2]) / sc.intr[0], (xa[:, 1] - sc.intr[3]) / sc.intr[1], np.ones(len(xa))], 1) * za[:, None]
    Xb = (Xa - T[:3]) @ rotation(T[3:])
    uv = np.stack([sc.intr[0] * Xb[:, 0] / Xb[:, 2] + sc.intr[2], sc.intr[1] * Xb[:, 1] / Xb[:, 2] + sc.intr[3]], 1)
    return dict(intr=sc.intr, T=T, A=(xa, za), B=(xb, np.full(len(xb), wrong)), truth=plane_depth(xb, sc.intr, pb, qb, sc.D),
                grad=plane_gradient(xb, sc.intr, pb, qb, sc.D), shift=float(np.abs(uv - xa).max()), H=H, W=W)


def property_figures(scene, m, radius):
    """(adopted share, largest relative depth error over the adopted keypoints divided by its bound (radius + 1) grad)."""
    ad = m["flags"] == ADOPTED
    err = np.abs(m["z_new"][ad] / scene["truth"][ad] - 1.0)
    return float(ad.mean()), float((err / ((radius + 1) * scene["grad"][ad])).max()) if ad.any() else 0.0


def property_share_bound(scene, radius):
    """A share that must adopt, by reasoning: A's grid of pitch 2 moves by at most `shift` pixels and nearly rigidly, so warped and
    rounded it leaves no gap wider than 3 < 2 radius + 1 pixels (radius >= 2) inside the image shrunk by ceil(shift) + 1; every
    keypoint of B inside that region has a carried neighbour, and with min_support = 1 a non-empty foreground adopts."""
    m = int(np.ceil(scene["shift"])) + 1
    xb = scene["B"][0]
    inside = (xb[:, 0] >= m) & (xb[:, 0] <= scene["W"] - 1 - m) & (xb[:, 1] >= m) & (xb[:, 1] <= scene["H"] - 1 - m)
    return float(inside.mean())
