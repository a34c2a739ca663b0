"""Roll-dominant splines: alignment problems whose consecutive knot rotations differ by ANY angle up to pi and still keep every
warp inside the keyframe (helper, no tests in it).

A large random rotation between two knots throws the warps out of the image and leaves nothing to compare.  A rotation about
(nearly) the optical axis through the principal point only turns the image about its centre, so keypoints in a disc round the
principal point stay in the image at every angle: the engine's pose entries (pose_entries.h: the per-knot and staged forms of
se3_math.h, the tabulated R * A) can then be held to the oracle at relative rotations where qlog / qexp leave their small-angle
ranges -- the series branches with a non-zero angle, relative w < 0, the |w| < 1e-10 branch of qlog, the upper reduction ranges
of fastm::atan_ratio / fastm::sincos."""
import numpy as np

import scenes
from mba_vo_amd import synth

# the relative angles between consecutive knots the pose-entry tests run: both sides of qlog's series threshold (sn = sin^2(a / 2)
# against 1e-20: a = 2e-10), the range the rest of the suite covers (<= 0.05), every reduction range of the atan (tan(a / 2) =
# 0.4375, 0.6875, 1.1875, 2.4375 at a = 0.82, 1.20, 1.74, 2.36) and, as "pi", the relative quaternion (axis, 0)
ANGLES = [1e-11, 1e-9, 3e-6, 1e-3, 0.05, 0.4, 1.1, 2.2, 2.9, 3.1, "pi"]


def angle_id(angle):
    return "pi" if angle == "pi" else "%g" % angle


def roll_knots(N, angle, rng, flip=False, exact_pi=False, tilt=0.03):
    """N rotation knots [N, 4] (xyzw): knot 0 the identity, knot i = knot i-1 * d_i with d_i a rotation by angle * U(0.7, 1.0)
    about normalize(e_z + tilt * N(0, I)).  exact_pi: d_i = (axis, 0) itself, so the relative quaternion's w comes out of the
    product as ~1e-17 (the |w| < 1e-10 branch of qlog).  flip: every odd knot negated -- the same rotations, relative w < 0.
    angle may be the string "pi" (= exact_pi)."""
    if isinstance(angle, str):
        assert angle == "pi"
        angle, exact_pi = np.pi, True
    q = np.zeros((N, 4))
    q[0] = [0.0, 0.0, 0.0, 1.0]
    for i in range(1, N):
        ax = np.array([0.0, 0.0, 1.0]) + tilt * rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = angle * rng.uniform(0.7, 1.0)
        d = np.r_[ax, 0.0] if exact_pi else np.r_[np.sin(0.5 * a) * ax, np.cos(0.5 * a)]
        q[i] = synth.quat_mul(q[i - 1], d)
    if flip:
        q[1::2] *= -1.0
    return np.ascontiguousarray(q)


def roll_scene(angle, k, S, F, seed, flip=False, exact_pi=False, H=120, W=160, K=80, tilt=0.03):
    """scenes.Scene (P = 8, trans_scale = 0.002: S = 32 stays on the spline; the scene's own N) with the rotation knots of
    roll_knots and integer keypoints uniformly in a disc of radius min(H, W) / 2 - 14 round (W / 2, H / 2)."""
    sc = scenes.Scene(H=H, W=W, S=S, F=F, k=k, P=8, K=K, seed=seed, trans_scale=0.002, rot_scale=0.0)
    rng = np.random.default_rng([seed, 7919])
    sc.knots_R = np.ascontiguousarray(roll_knots(sc.N, angle, rng, flip, exact_pi, tilt).ravel())
    r = (min(H, W) / 2.0 - 14.0) * np.sqrt(rng.uniform(0.0, 1.0, K))
    phi = rng.uniform(0.0, 2.0 * np.pi, K)
    sc.kp_xy = np.ascontiguousarray(np.stack([np.rint(W / 2.0 + r * np.cos(phi)), np.rint(H / 2.0 + r * np.sin(phi))], 1))
    return sc


def case_scene(angle, k, S, F, flip):
    """The scene of one test case: the seed depends on the angle, the degree and the flip only, so every S shares the knots."""
    return roll_scene(angle, k, S, F, seed=3000 + 10 * ANGLES.index(angle) + (2 if k == 4 else 0) + int(flip), flip=flip)


def branches(sc):
    """Which branch of qlog (se3_math.h) the relative quaternion conj(R_i) * R_i+1 of every consecutive knot pair takes, with
    qmul's own term order: "series" (sn < 1e-20), "pi" (|w| < 1e-10), else "general+" / "general-" by the sign of w."""
    q = sc.knots_R.reshape(-1, 4)
    out = []
    for a, b in zip(q[:-1], q[1:]):
        ax, ay, az, aw = -a[0], -a[1], -a[2], a[3]
        bx, by, bz, bw = b
        x = aw * bx + ax * bw + ay * bz - az * by
        y = aw * by + ay * bw + az * bx - ax * bz
        z = aw * bz + az * bw + ax * by - ay * bx
        w = aw * bw - ax * bx - ay * by - az * bz
        sn = x * x + y * y + z * z
        if sn < 1e-20:
            out.append("series")
        elif abs(w) < 1e-10:
            out.append("pi")
        else:
            out.append("general+" if w > 0 else "general-")
    return out
