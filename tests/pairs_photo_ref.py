"""numpy restatement of mbavo_pairs_match_brightness (include/mbavo.h, steps 1 - 8 and the correction) on one rebuilt entry (helper,
no test in it).

`entry` is what pairs_oracle.read_entry returns for one (pair, level).  The items are those of the depth evaluation's restatement
(tests/pairs_refine_ref.py: poses, pixels, the tap, Huber, patch_sum, lane_sum) without the gradient taps; the pyramid below a
corrected level 0 is synth.pyramid, the restatement tests/test_gpu_pairs_prep.py holds prepare and update to.  Everything is
float64, operation by operation as the header writes it; numpy contracts nothing and its division and rint are IEEE."""
import ctypes as C

import numpy as np

import pairs_refine_ref as ref
from mba_vo_amd import synth

E_RANGE, DEGENERATE = -2, 1
DEFAULTS = dict(rounds=3, min_pixels=64, min_var=4.0, gain_min=0.25, gain_max=4.0)
NAN = float("nan")


def items(e, pose_list):
    """Step 1: (s K x P, c K x P, valid K x P) -- the synthesised keyframe intensity, the current frame's grey level, validity."""
    K, P, S, H, W = e["K"], e["P"], e["S"], e["H"], e["W"]
    if K == 0:
        return np.zeros((0, P)), np.zeros((0, P)), np.zeros((0, P), bool)
    fx, fy, cx, cy = e["intr"]
    img = e["ref"] if e.get("word_I") is None else e["word_I"]
    px, py = ref.pixels(e, pose_list)
    inb = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    pxc, pyc = np.where(inb, px, 0), np.where(inb, py, 0)
    cur = e["curs"][0][pyc, pxc].astype(np.float64)
    xh, yh = (pxc - cx) / fx, (pyc - cy) / fy
    zh = 1.0 / np.sqrt((1. + xh * xh + yh * yh).astype(ref.F32)).astype(np.float64)
    ray = (xh * zh, yh * zh, zh)
    D = e["z"][:, None]
    iz = 1.0 / (D + 1e-8)
    ok, isum = inb.copy(), None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t, q in pose_list:
            R = ref.rotation_entries(q)
            rx = R[0] * ray[0] + R[1] * ray[1] + R[2] * ray[2]
            ry = R[3] * ray[0] + R[4] * ray[1] + R[5] * ray[2]
            rz = R[6] * ray[0] + R[7] * ray[1] + R[8] * ray[2]
            sc = (D - t[2]) * (1.0 / rz)
            Px, Py = sc * rx + t[0], sc * ry + t[1]
            tok, I, _, _, _ = ref._tap(img, e["grad"], H, W, (iz * fx) * Px + cx, (iz * fy) * Py + cy)
            ok &= tok
            isum = I if isum is None else isum + I
        s = np.where(ok, isum / float(ref.F32(S)), 0.0)
    return s, np.where(ok, cur, 0.0), ok


def sums(s, c, full, a, b, huber, P, cap):
    """Steps 2 - 4 under (a, b): (n, Sx, Sy, Sxx, Sxy, C)."""
    w, rho = ref.huber(c - (a * s + b), huber)
    ww = w * w
    terms = (ww, ww * s, ww * c, (ww * s) * s, (ww * s) * c, rho)
    return tuple(ref.lane_sum(np.where(full, ref.patch_sum(t), 0.0), P, cap) for t in terms)


def solve(n, Sx, Sy, Sxx, Sxy):
    """Step 5: (det, a, b)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n, Sx, Sy, Sxx, Sxy = (np.float64(v) for v in (n, Sx, Sy, Sxx, Sxy))
        det = n * Sxx - Sx * Sx
        a = (n * Sxy - Sx * Sy) / det
        return float(det), float(a), float((Sy - a * Sx) / n)


def fit_items(s, c, ok, P, cap, huber, rounds=0, min_pixels=0, min_var=0.0, gain_min=0.0, gain_max=0.0):
    """Steps 2 - 7 on the items of one (pair, level) with K rows: the record as a dict, and `trace` [(a_r, b_r, the six sums)]."""
    R = rounds or DEFAULTS["rounds"]
    min_pixels, min_var = min_pixels or DEFAULTS["min_pixels"], min_var or DEFAULTS["min_var"]
    gain_min, gain_max = gain_min or DEFAULTS["gain_min"], gain_max or DEFAULTS["gain_max"]
    full = ok.all(1) if len(ok) else np.zeros(0, bool)
    num_full = int(full.sum())
    out = dict(status=0, num_keypoints=len(ok), num_full=num_full, num_pixels=num_full * P, trace=[])
    a, b = 1.0, 0.0
    for r in range(R):
        v = sums(s, c, full, a, b, huber, P, cap)
        out["trace"].append((a, b, v))
        if r == 0:
            out["cost_before"] = v[5]
        det, a1, b1 = solve(*v[:5])
        n = np.float64(v[0])
        if out["num_pixels"] < min_pixels or not (det > (min_var * n) * n) or not np.isfinite(a1) or not np.isfinite(b1) or a1 < gain_min or a1 > gain_max:
            out.update(status=DEGENERATE, gain=1.0, offset=0.0, cost_after=out["cost_before"])
            return out
        a, b = a1, b1
    out.update(gain=a, offset=b, cost_after=sums(s, c, full, a, b, huber, P, cap)[5])
    return out


def fit(lib, capi, e, k, cap, huber=0.0, **opts):
    """The whole fit on one entry whose level has keypoint capacity `cap`."""
    if not ref.on_knots(e, k):
        return dict(status=E_RANGE, num_keypoints=e["K"], num_full=0, num_pixels=0, gain=NAN, offset=NAN, cost_before=NAN, cost_after=NAN)
    s, c, ok = items(e, ref.poses(lib, capi, e, k))
    return fit_items(s, c, ok, e["P"], cap, huber or e["huber"], **opts)


def correct(img, gain, offset):
    """The correction of a level-0 frame: min(255, max(0, rint((v - b) / a))), uint8."""
    v = np.rint((img.astype(np.float64) - np.float64(offset)) / np.float64(gain))
    return np.minimum(255.0, np.maximum(0.0, v)).astype(np.uint8)


def corrected_pyramid(img, gain, offset, L):
    """All L levels of a corrected frame, as mbavo_pairs_update with n_key = 0 makes them of the corrected level 0."""
    return synth.pyramid(np.ascontiguousarray(correct(img, gain, offset)), L)


def exposed(img, gain, offset):
    """A frame as a camera with that gain and offset would have taken it: clip(rint(a I + b))."""
    return np.clip(np.rint(np.float64(gain) * img.astype(np.float64) + np.float64(offset)), 0, 255).astype(np.uint8)


def opts_struct(capi, level=0, apply=0, rounds=0, min_pixels=0, huber=0.0, min_var=0.0, gain_min=0.0, gain_max=0.0):
    o = capi.PairsPhotoOpts()
    o.level, o.apply, o.rounds, o.min_pixels = level, apply, rounds, min_pixels
    o.huber, o.min_var, o.gain_min, o.gain_max = huber, min_var, gain_min, gain_max
    return o


def call(lib, handle, o, out=None):
    """The raw entry point with optional ctypes records."""
    return lib.mbavo_pairs_match_brightness(handle, None if o is None else C.byref(o), out)
