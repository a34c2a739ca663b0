"""The scene of the depth-refinement tests (helper, no test in it): three pairs of a workloads.RenderedScene at 64 x 48 (a textured
plane at z = 2, frames 0.1 apart, exposure 0.04, the ground-truth knots), rendered once on an MI355X and kept in
tests/golden/refine_scene.npz -- sharp keyframe, blurred current frame, float32 z-map, knots in the keyframe's camera, times.  The
depth maps are TRUE depths.  `entry` makes a level-0 entry on the host in the shape of pairs_oracle.read_entry; `oracle_quotient`
is the oracle's side of the derivative checks."""
import ctypes as C
import os

import numpy as np

import pairs_oracle as po
import pairs_refine_ref as ref
from mba_vo_amd import synth

B, H, W, S, K_DEG, N, HUBER = 3, 48, 64, 3, 4, 4, 10.0
INTR = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
DELTAS = (3e-4, 1e-3, 3e-3)
GAP = 0.1         # |g - oracle quotient| over the largest |g|, CPU, delta = 3e-3: 0.090 / 0.088 / 0.052 measured (profiles/r30_pairs_refine.txt)
_SCENE = {}


def scene():
    if not _SCENE:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_scene.npz"))
        for key in ("sharp", "blur", "depth", "kt", "kR", "times"):
            _SCENE[key] = np.stack([z["%s%d" % (key, b)] for b in range(B)])
    return _SCENE


def motion():
    """cap, exp, t0, dt, knots of the three pairs, as PairBatch.set_motion takes them."""
    c = scene()
    t = c["times"]
    return dict(cap=t[:, 1].copy(), exp=t[:, 2].copy(), t0=t[:, 0].copy(), dt=float(t[0, 3]), kt=c["kt"].copy(), kR=c["kR"].copy())


def gradient(img):
    """Central differences in float32, zero on the 1-pixel border (Gradient.h:56-71)."""
    f = img.astype(np.float32)
    g = np.zeros(img.shape + (2,), np.float32)
    g[1:-1, 1:-1, 0] = np.float32(0.5) * (f[1:-1, 2:] - f[1:-1, :-2])
    g[1:-1, 1:-1, 1] = np.float32(0.5) * (f[2:, 1:-1] - f[:-2, 1:-1])
    return g


def entry(b):
    """Pair b's level-0 entry: keypoints on a grid of 4, 8 pixels inside, with the z-map's depths."""
    c, m = scene(), motion()
    ys, xs = np.meshgrid(np.arange(8, H - 8, 4), np.arange(8, W - 8, 4), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    z = c["depth"][b][ys.ravel(), xs.ravel()].astype(np.float64)
    return dict(S=S, F=1, K=len(xy), P=8, k=K_DEG, N=N, H=H, W=W, fmt=0, ref=np.ascontiguousarray(c["sharp"][b]), word_I=None,
                grad=gradient(c["sharp"][b]), curs=[np.ascontiguousarray(c["blur"][b])], xy=xy, z=z, stride=2,
                pattern=np.ascontiguousarray(synth.PATTERN8, np.int32).ravel(), intr=INTR.copy(), cap=m["cap"][b:b + 1].copy(),
                exp=m["exp"][b:b + 1].copy(), t0=float(m["t0"][b]), dt=m["dt"], kt=np.ascontiguousarray(m["kt"][b]).ravel(),
                kR=np.ascontiguousarray(m["kR"][b]).ravel(), start=np.zeros(1, np.int32), huber=HUBER, outlier=None, num_bad=0)


def _oracle_pixels_and_costs(orc, e, z):
    """The oracle at depths z: (px, py K x P from ITS patch centres, unscaled patch costs K)."""
    L, dp = orc.lib(), orc.dp
    S_, K, P, k = e["S"], e["K"], e["P"], e["k"]
    q = dict(e, z=np.ascontiguousarray(z))
    poses = np.zeros(S_ * 7)
    L.orc_compute_virtual_camera_poses(S_, 1, dp(q["cap"]), dp(q["exp"]), k, q["t0"], q["dt"], dp(q["kt"]), dp(q["kR"]), dp(poses), None, None, None)
    centres = np.zeros(K * 2)
    L.orc_compute_local_patches_xy(S_, 1, dp(poses), dp(np.ascontiguousarray(q["xy"])), dp(q["z"]), K, dp(q["intr"]), dp(centres))
    pat = e["pattern"].reshape(-1, 2)
    cxy = centres.reshape(K, 2)
    px, py = np.trunc(cxy[:, :1] + pat[None, :, 0]).astype(np.int64), np.trunc(cxy[:, 1:] + pat[None, :, 1]).astype(np.int64)
    p, keep = po.problem_of(orc, q)
    _, costs = po.evaluate0(orc, p)
    return px, py, costs[0] * float(K * P)


def oracle_quotient(orc, lib, capi, e, delta):
    """K P (c_i(D + delta) - c_i(D - delta)) / (2 delta) from the oracle's patch costs (a patch depends on its own depth only, so
    all depths move at once), the same at 2 delta, and the keypoints that qualify: the P truncated pixels of the ORACLE's patch
    centres are the same at D - 2 delta .. D + 2 delta and all valid there (validity: the evaluation's rule, restated)."""
    z = e["z"]
    at = [_oracle_pixels_and_costs(orc, e, z + s * delta) for s in (-2, -1, 0, 1, 2)]
    pl = ref.poses(lib, capi, e, e["k"])
    same = np.ones(e["K"], bool)
    for (px, py, _), s in zip(at, (-2, -1, 0, 1, 2)):
        same &= (px == at[2][0]).all(1) & (py == at[2][1]).all(1)
        same &= ref.keypoints(e, pl, z=z + s * delta, px_py=(at[2][0], at[2][1]))["full"]
    q1 = (at[3][2] - at[1][2]) / (2 * delta)
    q2 = (at[4][2] - at[0][2]) / (4 * delta)
    return q1, q2, same


def quotient_bound(e, r, q1, q2, delta):
    """What |g - q(delta)| may be, from the quotient's own terms and the gradient image's mismatch: truncation 3 |q(2 delta) -
    q(delta)| (smooth pieces: q(2d) - q(d) = 3 (q(d) - c') + O(d^4); a tap that crosses a pixel boundary inside the stencil: O(d)
    in both); rounding e_c / delta with e_c = P a 9 * 255 * 2^-24 + c 2^-23 (float32 blends and square roots); model: r["model"]."""
    e_c = e["P"] * e["huber"] * 9 * 255.0 * 2.0 ** -24 + r["rho_sum"] * 2.0 ** -23
    return 3 * np.abs(q2 - q1) + e_c / delta + r["model"]
