"""numpy restatement of mbavo_pairs_refine_depths (include/mbavo.h, steps 1 - 9) on one rebuilt entry (helper, no test in it).

`entry` is what pairs_oracle.read_entry returns for one (pair, level): everything an mbavo_problem points at.  The pose of a
sample comes from the library's host spline (mbavo_spline_get_pose: the same algebra as the device's prologue, rounded in another
order).  The fp32 islands are mirrored in float32: unit_ray's sqrtf, the bilinear blend's weights and sums, Huber's two sqrtf.
Everything else is float64, operation by operation as the header writes it."""
import ctypes as C

import numpy as np

F32 = np.float32
E_RANGE = -2


def sample_times(cap, exp, S):
    return [cap - exp * 0.5 + s * exp / (S - 1 + 1e-8) for s in range(S)]


def on_knots(e, k):
    for t in sample_times(float(e["cap"][0]), float(e["exp"][0]), e["S"]):
        tn = (t - e["t0"]) / e["dt"]
        if not (t == t) or int(tn) < 0 or int(tn) + k > e["N"]:
            return False
    return True


def poses(lib, capi, e, k):
    """[(t (3), q xyzw (4))] of the S samples."""
    kt, kR = np.ascontiguousarray(e["kt"], np.float64), np.ascontiguousarray(e["kR"], np.float64)
    out = []
    for t in sample_times(float(e["cap"][0]), float(e["exp"][0]), e["S"]):
        p, q = np.zeros(3), np.zeros(4)
        assert lib.mbavo_spline_get_pose(k, e["t0"], e["dt"], capi.dp(kt), capi.dp(kR), e["N"], float(t), capi.dp(p), capi.dp(q), None, None) == 0
        out.append((p, q))
    return out


def rotation_entries(q):
    qx, qy, qz, qw = q
    return np.array([qw * qw + qx * qx - qy * qy - qz * qz, -2. * (qw * qz - qx * qy), 2. * (qw * qy + qx * qz),
                     2. * (qw * qz + qx * qy), qw * qw - qx * qx + qy * qy - qz * qz, -2. * (qw * qx - qy * qz),
                     -2. * (qw * qy - qx * qz), 2. * (qw * qx + qy * qz), qw * qw - qx * qx - qy * qy + qz * qz])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz)


def _qrotate(q, p):
    c = (-q[0], -q[1], -q[2], q[3])
    v = _qmul(_qmul(q, (p[0], p[1], p[2], 0.0 * p[0])), c)
    return v[0], v[1], v[2]


def patch_centres(t, q, xy, z, intr):
    """patch_centre_rt at the pose (t, q), for all keypoints at once."""
    fx, fy, cx, cy = intr
    r2c = (-q[0], -q[1], -q[2], q[3])
    rt = _qrotate(r2c, (np.float64(t[0]), np.float64(t[1]), np.float64(t[2])))
    P = (z * (xy[:, 0] - cx) / fx, z * (xy[:, 1] - cy) / fy, z)
    rp = _qrotate(r2c, P)
    X, Y, Z = rp[0] - rt[0], rp[1] - rt[1], rp[2] - rt[2]
    return X / Z * fx + cx, Y / Z * fy + cy


def _tap(img, grad, H, W, x, y):
    """tap_fetch + tap_blend with gradients: (ok, I, gx, gy, (sx, sy)), float32 weights and accumulation; (sx, sy) is the slope of
    the bilinear interpolant at the tap, which the interpolated central differences (gx, gy) only approximate."""
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    xi, yi = np.minimum(xs.astype(np.int64), W - 2), np.minimum(ys.astype(np.int64), H - 2)
    dx, dy = (xs - xi).astype(F32), (ys - yi).astype(F32)
    dxdy = dx * dy
    w00, w01, w10, w11 = F32(1.0) - dx - dy + dxdy, dx - dxdy, dy - dxdy, dxdy

    def blend(a):
        v = w11 * a[yi + 1, xi + 1]
        v = v + w10 * a[yi + 1, xi]
        v = v + w01 * a[yi, xi + 1]
        v = v + w00 * a[yi, xi]
        return v.astype(np.float64)
    f = img.astype(np.float64)
    i00, i01, i10, i11 = f[yi, xi], f[yi, xi + 1], f[yi + 1, xi], f[yi + 1, xi + 1]
    fx_, fy_ = (xs - xi), (ys - yi)
    slope = ((1 - fy_) * (i01 - i00) + fy_ * (i11 - i10), (1 - fx_) * (i10 - i00) + fx_ * (i11 - i01))  # of the bilinear interpolant itself
    return ok, blend(img.astype(F32)), blend(grad[:, :, 0].astype(F32)), blend(grad[:, :, 1].astype(F32)), slope


def huber(r, a):
    aa, x = a * a, 0.5 * r * r
    sx = np.sqrt(x.astype(F32)).astype(np.float64)
    hub = x > aa
    w = np.where(hub, np.sqrt((a / (sx + 1e-8)).astype(F32)).astype(np.float64), 1.0)
    return w, np.where(hub, 2 * a * sx - aa, x)


def patch_sum(v):
    """patch_rho_sum along the last axis: the stride-halving tree for a power-of-two P, the ascending sum otherwise."""
    P = v.shape[-1]
    if P & (P - 1) == 0:
        b = v.copy()
        s = P // 2
        while s >= 1:
            b = b[..., :s] + b[..., s:2 * s]
            s //= 2
        return b[..., 0]
    acc = np.zeros(v.shape[:-1])
    for p in range(P):
        acc = acc + v[..., p]
    return acc


def pixels(e, pose_list, z=None):
    """Step 1 and the truncation of step 2: (px, py) K x P int64, at depths z (default: the entry's)."""
    z = e["z"] if z is None else z
    t, q = pose_list[e["S"] // 2]
    ox, oy = patch_centres(t, q, e["xy"], z, e["intr"])
    pat = e["pattern"].reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return np.trunc(ox[:, None] + pat[None, :, 0]).astype(np.int64), np.trunc(oy[:, None] + pat[None, :, 1]).astype(np.int64)


def keypoints(e, pose_list, z=None, px_py=None):
    """Steps 2 - 6 for every keypoint: dict(g, h, cost (K), valid (K int), full (K bool), rho_sum (K: sum_j rho_j whatever valid
    is), px, py, model (K: a bound on |g - derivative of the interpolated cost|), rim (K: the smallest distance, in pixels, of any
    tap of the keypoint's pixels that lie in the current image from the bounds 0, W - 1, H - 1 of the tap test)).  z: the depths (default: the entry's); px_py: pixels held fixed (default: those of z)."""
    z = np.asarray(e["z"] if z is None else z, np.float64)
    K, P, S, H, W = e["K"], e["P"], e["S"], e["H"], e["W"]
    fx, fy, cx, cy = e["intr"]
    img = e["ref"] if e.get("word_I") is None else e["word_I"]
    px, py = pixels(e, pose_list, z) if px_py is None else px_py
    if K == 0:
        zero = np.zeros(0)
        return dict(g=zero, h=zero, cost=zero, valid=np.zeros(0, np.int32), full=np.zeros(0, bool), rho_sum=zero, px=px, py=py, model=zero, rim=zero)
    inb = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    pxc, pyc = np.where(inb, px, 0), np.where(inb, py, 0)
    cur = e["curs"][0][pyc, pxc].astype(np.float64)
    xh, yh = (pxc - cx) / fx, (pyc - cy) / fy
    zh = 1.0 / np.sqrt((1. + xh * xh + yh * yh).astype(F32)).astype(np.float64)
    ray = (xh * zh, yh * zh, zh)
    D = z[:, None]
    iz = 1.0 / (D + 1e-8)
    ok, isum, acc, mis = inb.copy(), None, np.zeros((K, P)), np.zeros((K, P))
    rim = np.full((K, P), np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t, q in pose_list:
            R = rotation_entries(q)
            rx = R[0] * ray[0] + R[1] * ray[1] + R[2] * ray[2]
            ry = R[3] * ray[0] + R[4] * ray[1] + R[5] * ray[2]
            rz = R[6] * ray[0] + R[7] * ray[1] + R[8] * ray[2]
            C1 = 1.0 / rz
            sc = (D - t[2]) * C1
            Px, Py = sc * rx + t[0], sc * ry + t[1]
            u, v = (iz * fx) * Px + cx, (iz * fy) * Py + cy
            tok, I, gx, gy, (sx, sy) = _tap(img, e["grad"], H, W, u, v)
            ok &= tok
            for c, hi in ((u, W - 1), (v, H - 1)):
                rim = np.fmin(rim, np.fmin(np.abs(c), np.abs(c - hi)))
            isum = I if isum is None else isum + I
            du = fx * (((C1 * rx) * iz) - ((Px * iz) * iz))
            dv = fy * (((C1 * ry) * iz) - ((Py * iz) * iz))
            acc = acc + (gx * du + gy * dv)
            mis = mis + (np.abs(gx - sx) * np.abs(du) + np.abs(gy - sy) * np.abs(dv))
        fS = float(F32(S))
        res = np.where(ok, isum / fS - cur, 0.0)
        d = np.where(ok, (1.0 / fS) * acc, 0.0)
    w, rho = huber(res, e["huber"])
    ww = w * w
    valid = ok.sum(1).astype(np.int32)
    full = valid == P
    rho_sum = patch_sum(rho)
    # |g - the derivative of the cost as the interpolant has it| <= model: the gradient image's mismatch, pixel by pixel
    model = (ww * np.abs(res) * np.where(ok, (1.0 / fS) * mis, 0.0)).sum(1)
    return dict(g=np.where(full, patch_sum((ww * res) * d), 0.0), h=np.where(full, patch_sum((ww * d) * d), 0.0),
                cost=np.where(full, rho_sum, 0.0), valid=valid, full=full, rho_sum=rho_sum, px=px, py=py, model=model,
                rim=np.where(inb, rim, np.inf).min(1))


def lane_sum(terms, P, cap):
    """Step 9: tiles of T = min(256, 1024 // P) keypoints, G = min(64, max(1, ceil(cap / T))) workgroups, workgroup w takes tiles w,
    w + G, ..; a lane adds its terms in ascending order from 0.0; butterfly within each wave, the four waves in order; with G > 1
    the G workgroup sums from 0.0 in the order of w."""
    T = min(256, 1024 // P)
    G = min(64, max(1, -(-cap // T)))
    lanes = np.zeros((G, 256))
    for kp, v in enumerate(terms):
        w, i = (kp // T) % G, kp % T
        lanes[w, i] = lanes[w, i] + v
    sums = []
    for w in range(G):
        x = lanes[w].reshape(4, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            x = x + x[:, np.arange(64) ^ off]
        sums.append(((x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0])
    if G == 1:
        return float(sums[0])
    acc = 0.0
    for v in sums:
        acc = acc + v
    return float(acc)


def step(z, g, h, full, min_info=0.0, max_rel_step=0.0, z_min=0.0, z_max=0.0):
    """Step 7: (moved K bool, z_new K (z where not moved), rel K (d_rho / rho, 0 where not moved), h_rho K)."""
    max_rel_step = 0.25 if max_rel_step == 0 else max_rel_step
    z_min = 1e-2 if z_min == 0 else z_min
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rho, DD = 1.0 / z, z * z
        g_rho, h_rho = -(DD * g), (DD * DD) * h
        cand = full & (h_rho > min_info) & (h_rho > 0.0)
        m = max_rel_step * rho
        d_rho = -g_rho / h_rho
        d_rho = np.where(d_rho > m, m, d_rho)
        d_rho = np.where(d_rho < -m, -m, d_rho)
        z_new = 1.0 / (rho + d_rho)
        moved = cand & np.isfinite(z_new) & (z_new >= z_min) & ((z_max == 0) | (z_new <= z_max))
        rel = np.where(moved, d_rho / rho, 0.0)
    return moved, np.where(moved, z_new, z), rel, h_rho


def refine(lib, capi, e, k, cap, **opts):
    """The whole call on one entry whose level has keypoint capacity `cap`: dict(status, record fields, g, h, cost, valid, moved, z_new, h_rho)."""
    if not on_knots(e, k):
        return dict(status=E_RANGE, num_keypoints=e["K"], num_full=0, num_moved=0, cost=float("nan"), sum_sq_rel=float("nan"))
    r = keypoints(e, poses(lib, capi, e, k))
    moved, z_new, rel, h_rho = step(e["z"], r["g"], r["h"], r["full"], **opts)
    P = e["P"]
    r.update(status=0, num_keypoints=e["K"], num_full=int(r["full"].sum()), num_moved=int(moved.sum()),
             sum_cost=lane_sum(np.where(r["full"], r["cost"], 0.0), P, cap), sum_sq_rel=lane_sum(np.where(moved, rel * rel, 0.0), P, cap),
             moved=moved, z_new=z_new, rel=rel, h_rho=h_rho)
    return r


def opts_struct(capi, level=0, apply=0, min_info=0.0, max_rel_step=0.0, z_min=0.0, z_max=0.0):
    o = capi.PairsRefineOpts()
    o.level, o.apply, o.min_info, o.max_rel_step, o.z_min, o.z_max = level, apply, min_info, max_rel_step, z_min, z_max
    return o


def call(lib, handle, o, out=None, g=None, h=None, cost=None, valid=None):
    """The raw entry point with optional ctypes records and device pointers (ints)."""
    return lib.mbavo_pairs_refine_depths(handle, None if o is None else C.byref(o), out, g, h, cost, valid)
