"""The pairs tracker's pose algebra in exact arithmetic (helper, no tests in it): shared by tests/test_pose_algebra_ref.py (CPU) and
tests/test_gpu_pairs_pose_angles.py (GPU).

Everything the tracker-state kernels compute with se3_math.h / pose_math.h -- quaternion product and rotation, Core::Transformation
make / inverse / multiply, the SE(3) exponential and logarithm, SplineSE3::TransformByRight, TransformTo(cap, identity) and
SplineSE3::GetPose for k = 2 and k = 4 -- restated in Python's `decimal` at PREC digits with its own sine, cosine and arctangent
(Taylor series after argument reduction), so a GPU test needs nothing but the standard library.  These are the TRUE functions: no
series branch, no threshold.  The only convention is the reference's for the logarithm: theta = 2 atan(n / w) in (-pi, pi), and
w == 0 gives -pi (Quaternion.h:100-112, Sophus::SO3::log as Transformation::log uses it).  Inputs are doubles converted exactly;
results are rounded to double once, at the end (`to_float`).

Where a kernel forms a number in double before the algebra, the case builders form it with the same IEEE operations in Python floats:
velocity * dt_frame, (s * velocity) * dt_frame + twist, dt_frame = cap - prev_timestamp, t0 = cap - exp / 2 and the spline's
normalised time u = (t - t0) / dt - idx.

The bound of the GPU file, per quantity and case: |device - exact| <= 4 * max(host_err[quantity][case], floor[quantity]) where
host_err is |C ABI host algebra - exact| on the same case and floor[quantity] the largest host_err over the cases with an angle in
[1e-2, 2.9], where no cancellation plays a part.  Both are computed on the CPU (`predict_host`, `commit_host`, `bounds`); nothing comes from the device."""
import decimal
from decimal import Decimal as Dec

import numpy as np

PREC = 60  # working digits (the issue asks for 50; ten guard digits)
CTX = decimal.Context(prec=PREC, rounding=decimal.ROUND_HALF_EVEN, Emin=-999999999, Emax=999999999)
decimal.setcontext(CTX)  # (operators on Decimal, a unary minus among them, round to the thread's context: 28 digits by default)
ALGEBRA_CAP = 1e-9
BAND = (1e-10, 1e-3)       # the cancellation band of se3_exp's c1 / c2: bounds of cases at or above BAND[1] must stay under ALGEBRA_CAP
FLOOR_RANGE = (1e-2, 2.9)  # the angles the floor of a quantity is taken over
PI_F = float(np.pi)
# the issue's angles; "pi" (the relative quaternion (axis, 0), w == 0 exactly) is for the logarithm only.  1.1 and 2.2 are added:
# fastm::atan_ratio reduces tan(a / 2) in five ranges (limits 0.4375, 0.6875, 1.1875, 2.4375: a = 0.82, 1.20, 1.74, 2.36) and the
# issue's list has no angle in the second and the fourth, so a wrong constant there would pass (the sensitivity check of the issue)
ANGLES = [1e-11, 0.99e-10, 1.01e-10, 1e-9, 1.5e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-2, 0.4, 1.1, 1.6, 2.2, 2.9, 3.1, PI_F - 1e-11]
LOG_ANGLES = ANGLES + ["pi"]
ZERO, ONE, TWO, HALF = Dec(0), Dec(1), Dec(2), Dec("0.5")


def angle_id(a):
    return "pi" if isinstance(a, str) else ("pi-1e-11" if a == ANGLES[-1] else "%g" % a)


def angle_value(a):
    return PI_F if isinstance(a, str) else float(a)


# ---------------------------------------------------------------------------------------------------------------- scalars
def D(x):
    """A double (or int), exactly."""
    return x if isinstance(x, Dec) else Dec(float(x))


def vec(a):
    return [D(v) for v in np.asarray(a, dtype=np.float64).ravel().tolist()]


def to_float(a):
    """Rounded to double: a scalar or a (nested) list."""
    if isinstance(a, Dec):
        return float(a)
    return np.array([to_float(v) for v in a], dtype=np.float64)


def add(a, b): return CTX.add(a, b)
def sub(a, b): return CTX.subtract(a, b)
def mul(a, b): return CTX.multiply(a, b)
def div(a, b): return CTX.divide(a, b)
def sqrt(a): return CTX.sqrt(a)


def _atan_series(x):
    """sum (-1)^i x^(2i+1) / (2i+1), |x| <= 0.2."""
    x2, term, total, i = mul(x, x), x, x, 1
    tiny = Dec(10) ** (-(PREC + 5))
    while True:
        term = CTX.minus(mul(term, x2))
        step = div(term, Dec(2 * i + 1))
        total = add(total, step)
        if abs(step) <= tiny * max(abs(total), tiny):
            return total
        i += 1


def _machin_pi():
    return sub(mul(Dec(16), _atan_series(div(ONE, Dec(5)))), mul(Dec(4), _atan_series(div(ONE, Dec(239)))))


PI = _machin_pi()


def atan(x):
    """Arctangent: odd, |x| > 1 through pi / 2 - atan(1 / x), then halvings atan(x) = 2 atan(x / (1 + sqrt(1 + x^2))) to |x| <= 0.2."""
    if x < 0:
        return CTX.minus(atan(CTX.minus(x)))
    if x > 1:
        return sub(div(PI, TWO), atan(div(ONE, x)))
    k = 0
    while x > Dec("0.2"):
        x = div(x, add(ONE, sqrt(add(ONE, mul(x, x)))))
        k += 1
    return mul(_atan_series(x), Dec(2 ** k))


def sincos(x):
    """(sin x, cos x): x reduced by multiples of 2 pi to [-pi, pi], halved eight times, Taylor series, eight double-angle steps."""
    two_pi = mul(TWO, PI)
    if abs(x) > PI:
        x = sub(x, mul(two_pi, CTX.to_integral_value(div(x, two_pi))))
    h = 8
    y = div(x, Dec(2 ** h))
    y2 = mul(y, y)
    tiny = Dec(10) ** (-(PREC + 5))
    s, c, ts, tc, i = y, ONE, y, ONE, 1
    while True:
        tc = CTX.minus(div(mul(tc, y2), Dec((2 * i - 1) * (2 * i))))
        ts = CTX.minus(div(mul(ts, y2), Dec((2 * i) * (2 * i + 1))))
        s, c = add(s, ts), add(c, tc)
        if abs(tc) <= tiny and abs(ts) <= tiny:
            break
        i += 1
    # (the plain recurrences: eight steps lose a few of the guard digits at most)
    for _ in range(h):
        s, c = mul(TWO, mul(s, c)), sub(mul(c, c), mul(s, s))
    return s, c


# ---------------------------------------------------------------------------------------------------------------- quaternions (xyzw)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [sub(add(add(mul(aw, bx), mul(ax, bw)), mul(ay, bz)), mul(az, by)),
            sub(add(add(mul(aw, by), mul(ay, bw)), mul(az, bx)), mul(ax, bz)),
            sub(add(add(mul(aw, bz), mul(az, bw)), mul(ax, by)), mul(ay, bx)),
            sub(sub(sub(mul(aw, bw), mul(ax, bx)), mul(ay, by)), mul(az, bz))]


def qconj(a):
    return [CTX.minus(a[0]), CTX.minus(a[1]), CTX.minus(a[2]), a[3]]


def qrot(q, p):
    """q * (p, 0) * conj(q) (Quaternion.h:53-60): for a q that is not exactly of unit length this scales by |q|^2, as the code does."""
    return qmul(qmul(q, [p[0], p[1], p[2], ZERO]), qconj(q))[:3]


def norm2(v):
    s = ZERO
    for x in v:
        s = add(s, mul(x, x))
    return s


def qlog(q):
    """Quaternion.h:61-157 without its branches: 2 atan(n / w) / n * (x, y, z); w == 0: -pi / n."""
    n2 = norm2(q[:3])
    if n2 == 0:
        return [ZERO, ZERO, ZERO]
    n = sqrt(n2)
    theta = CTX.minus(PI) if q[3] == 0 else mul(TWO, atan(div(n, q[3])))
    lam = div(theta, n)
    return [mul(lam, q[0]), mul(lam, q[1]), mul(lam, q[2])]


def qexp(tg):
    """Quaternion.h:159-233: (sin(theta / 2) / theta * tg, cos(theta / 2))."""
    th2 = norm2(tg)
    if th2 == 0:
        return [ZERO, ZERO, ZERO, ONE]
    th = sqrt(th2)
    s, c = sincos(mul(HALF, th))
    im = div(s, th)
    return [mul(im, tg[0]), mul(im, tg[1]), mul(im, tg[2]), c]


# ---------------------------------------------------------------------------------------------------------------- Core::Transformation
IDENTITY = [ZERO, ZERO, ZERO, ZERO, ZERO, ZERO, ONE]


def make(q, t):
    """Transformation(q, t): the quaternion normalised (Eigen normalized())."""
    z = norm2(q)
    if z > 0:
        n = sqrt(z)
        q = [div(v, n) for v in q]
    return [t[0], t[1], t[2], q[0], q[1], q[2], q[3]]


def inverse(T):
    qc = qconj(T[3:])
    return make(qc, qrot(qc, [CTX.minus(T[0]), CTX.minus(T[1]), CTX.minus(T[2])]))


def tmul(A, B):
    a = A[3:]
    t = qrot(a, B[:3])
    return make(qmul(a, B[3:]), [add(t[0], A[0]), add(t[1], A[1]), add(t[2], A[2])])


def _hat(w):
    return [[ZERO, CTX.minus(w[2]), w[1]], [w[2], ZERO, CTX.minus(w[0])], [CTX.minus(w[1]), w[0], ZERO]]


def _mat_apply(c0, c1, c2, w, v):
    """(c0 I + c1 hat(w) + c2 hat(w)^2) v."""
    O = _hat(w)
    Ov = [add(add(mul(O[r][0], v[0]), mul(O[r][1], v[1])), mul(O[r][2], v[2])) for r in range(3)]
    OOv = [add(add(mul(O[r][0], Ov[0]), mul(O[r][1], Ov[1])), mul(O[r][2], Ov[2])) for r in range(3)]
    return [add(add(mul(c0, v[r]), mul(c1, Ov[r])), mul(c2, OOv[r])) for r in range(3)]


def se3_exp(a):
    """Transformation::exp -> Sophus::SE3d::exp: (V(omega) upsilon, exp(omega)), V = I + (1 - cos) / th^2 hat + (th - sin) / th^3 hat^2."""
    ups, om = a[:3], a[3:]
    th2 = norm2(om)
    if th2 == 0:
        return make([ZERO, ZERO, ZERO, ONE], list(ups))
    th = sqrt(th2)
    s, c = sincos(th)
    # 1 - cos(th) = 2 sin^2(th / 2): exact arithmetic would not need it, PREC digits at th = 1e-11 do
    sh, _ = sincos(mul(HALF, th))
    c1 = div(mul(TWO, mul(sh, sh)), th2)
    c2 = div(sub(th, s), mul(th2, th))
    return make(qexp(om), _mat_apply(ONE, c1, c2, om, ups))


def se3_log(T):
    """Transformation::log -> Sophus::SE3d::log: omega = theta * axis with the convention above, upsilon = V^-1 t with
    V^-1 = I - hat / 2 + (1 - theta cos(theta / 2) / (2 sin(theta / 2))) / theta^2 hat^2."""
    q, t = T[3:], T[:3]
    om = qlog(q)
    th2 = norm2(om)
    if th2 == 0:
        return [t[0], t[1], t[2], ZERO, ZERO, ZERO]
    th = sqrt(th2)  # (the coefficient is even in theta)
    s, c = sincos(mul(HALF, th))
    c2 = div(sub(ONE, div(mul(th, c), mul(TWO, s))), th2)
    return _mat_apply(ONE, CTX.minus(HALF), c2, om, t) + om


# ---------------------------------------------------------------------------------------------------------------- SplineSE3
def transform_by_right(kt, kR, q, t):
    """Spline.h:212-219: t_i += R_i * t, R_i = R_i * q.  kt: N x 3, kR: N x 4 lists."""
    out_t, out_R = [], []
    for ti, Ri in zip(kt, kR):
        r = qrot(Ri, t)
        out_t.append([add(ti[0], r[0]), add(ti[1], r[1]), add(ti[2], r[2])])
        out_R.append(qmul(Ri, q))
    return out_t, out_R


def segment(t, t0, dt):
    """SplineFunctor.h:13-19 in doubles, as every implementation forms it: (idx, u)."""
    tn = (float(t) - float(t0)) / float(dt)
    idx = int(tn)
    return idx, tn - idx


def get_pose(k, kt, kR, idx, u):
    """SplineSE3::GetPose (SplineFunctor.h:21-94, 155-365 / oracle/mbavo_oracle.c: orc_c2_vec3, orc_c4_vec3, orc_c2_rot3,
    orc_c4_rot3) on knots idx .. idx + k - 1 at the normalised time u (a double): (p, q), q not normalised."""
    u = D(u)
    t, R = kt[idx:idx + k], kR[idx:idx + k]
    if k == 2:
        cs = [sub(ONE, u), u]
        ws = [u]
    else:
        uu = mul(u, u)
        uuu = mul(uu, u)
        s = div(ONE, Dec(6))
        cs = [add(sub(s, mul(HALF, u)), sub(mul(HALF, uu), mul(s, uuu))), add(sub(mul(Dec(4), s), uu), mul(HALF, uuu)),
              sub(add(add(s, mul(HALF, u)), mul(HALF, uu)), mul(HALF, uuu)), mul(s, uuu)]
        ws = [add(sub(add(mul(Dec(5), s), mul(HALF, u)), mul(HALF, uu)), mul(s, uuu)),
              sub(add(add(s, mul(HALF, u)), mul(HALF, uu)), mul(mul(TWO, s), uuu)), mul(s, uuu)]
    p = [ZERO, ZERO, ZERO]
    for c, tj in zip(cs, t):
        p = [add(p[a], mul(c, tj[a])) for a in range(3)]
    q = R[0]
    for g, w in enumerate(ws):
        om = qlog(qmul(qconj(R[g]), R[g + 1]))
        q = qmul(q, qexp([mul(w, v) for v in om]))
    return p, q


def transform_to_identity(kt, kR, p, q):
    """SplineSE3::TransformTo(cap, identity) (Spline.h:183-200) given GetPose(cap) = (p, q): dR = q^-1 (Eigen inverse(): conjugate /
    squared norm), dt = q^-1 * (0 - p), then TransformByRight."""
    n2 = norm2(q)
    qi = [div(v, n2) for v in qconj(q)]
    d = [CTX.minus(p[0]), CTX.minus(p[1]), CTX.minus(p[2])]
    return transform_by_right(kt, kR, qmul(qi, [ZERO, ZERO, ZERO, ONE]), qrot(qi, d))


# ---------------------------------------------------------------------------------------------------------------- the kernels, exact
def tangent(velocity, dt_frame, scale=None, twist=None):
    """The tangent as the kernels form it in double: velocity * dt_frame, or (s * velocity) * dt_frame + twist (6 Python floats)."""
    if scale is None:
        return [float(v) * float(dt_frame) for v in velocity]
    return [(float(scale) * float(v)) * float(dt_frame) + float(tw) for v, tw in zip(velocity, twist)]


def knot_lists(kt, kR):
    kt, kR = np.asarray(kt, np.float64).reshape(-1, 3), np.asarray(kR, np.float64).reshape(-1, 4)
    return [vec(r) for r in kt], [vec(r) for r in kR]


def predict(kt, kR, tan):
    """k_pairs_predict / k_pairs_hypotheses on one pair: TransformByRight(exp(tan)) -> (kt N x 3, kR N x 4) Decimal lists."""
    dT = se3_exp(vec(tan))
    t, R = knot_lists(kt, kR)
    return transform_by_right(t, R, dT[3:], dT[:3])


def commit(k, kt, kR, t0, dt, cap, T_prev, T_keyframe, dt_frame, verdict):
    """k_pairs_commit on one pair.  kt, kR: Decimal knot lists (after the predict); t0: the spline's start as published (a double);
    T_prev, T_keyframe: 7 doubles; dt_frame a double.  Returns a dict of Decimal lists: T (GetPose at cap), velocity, T_prev,
    T_keyframe, knots_t, knots_R (flat), T_world."""
    idx, u = segment(cap, t0, dt)
    p, q = get_pose(k, kt, kR, idx, u)
    Tb = make(q, p)
    Tk = vec(T_keyframe)
    lg = se3_log(tmul(inverse(vec(T_prev)), Tb))
    out = dict(T=p + q, velocity=[div(v, D(dt_frame)) for v in lg], T_prev=Tb, T_keyframe=Tk)
    if verdict:
        out["T_keyframe"] = tmul(Tk, Tb)
        out["T_prev"] = list(IDENTITY)
        kt, kR = transform_to_identity(kt, kR, p, q)
    p2, q2 = get_pose(k, kt, kR, idx, u)
    out["T_world"] = tmul(out["T_keyframe"], make(q2, p2))
    out["knots_t"] = [v for r in kt for v in r]
    out["knots_R"] = [v for r in kR for v in r]
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
N_KNOTS, DT, H, W, K_POINTS, DISC = 6, 0.5, 120, 160, 40, 30.0
INTR = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _quat(axis, angle):
    return np.r_[np.sin(0.5 * angle) * _unit(axis), np.cos(0.5 * angle)]


def _np_qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def roll_axis(rng, tilt=0.03):
    """tests/roll_scenes.roll_knots's axis: nearly the optical axis, so that a rotation of any angle keeps a central disc in view."""
    return _unit(np.array([0.0, 0.0, 1.0]) + tilt * rng.normal(size=3))


def slow_knots(rng, sign=1.0):
    """N ordinary knots: translations of ~0.1, rotations a few hundredths of a radian apart round a random small rotation."""
    kt = 0.1 * rng.normal(size=(N_KNOTS, 3))
    kR = np.zeros((N_KNOTS, 4))
    q = _quat(rng.normal(size=3), 0.05 * rng.uniform())
    for i in range(N_KNOTS):
        kR[i] = q
        q = _np_qmul(q, _quat(rng.normal(size=3), 0.02))
    return kt, sign * kR


def roll_knots(rng, angle, flip, tilt=0.03):
    """tests/roll_scenes.roll_knots with the relative angle EXACTLY `angle` (not scaled): knot 0 the identity, knot i = knot i-1 * d_i
    with d_i the rotation by `angle` about roll_axis; flip: every odd knot negated (relative w < 0)."""
    kR = np.zeros((N_KNOTS, 4))
    kR[0] = [0.0, 0.0, 0.0, 1.0]
    for i in range(1, N_KNOTS):
        kR[i] = _np_qmul(kR[i - 1], _quat(roll_axis(rng, tilt), angle))
    if flip:
        kR[1::2] *= -1.0
    return kR


def times(i):
    """(cap, exp) of pair i: u = exp / (2 dt) after the predict takes 0.04, 0.2 and 0.45 in turn."""
    return 0.55 + 0.013 * (i % 11), (0.04, 0.2, 0.45)[i % 3]


def disc_points(rng, n=K_POINTS, radius=DISC):
    """Whole-pixel keypoints in a disc round the principal point with depths in [2, 3]: (xy n x 2, z n)."""
    r = radius * np.sqrt(rng.uniform(0.0, 1.0, n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    xy = np.stack([np.rint(W / 2.0 + r * np.cos(phi)), np.rint(H / 2.0 + r * np.sin(phi))], 1)
    return np.ascontiguousarray(xy), np.ascontiguousarray(rng.uniform(2.0, 3.0, n))


def case_points(i):
    """The keypoints of pair i of every check."""
    return disc_points(np.random.default_rng([2829, i]))


def _translation(rng):
    """A translation part of ordinary size: |upsilon| in [0.03, 0.3]."""
    return _unit(rng.normal(size=3)) * rng.uniform(0.03, 0.3)


def exp_cases(roll=False, seed=0):
    """One pair per (angle, knot sign): dict(angle, sign, kt, kR, tan6 (the intended tangent), cap, exp, prev).  roll: the rotation
    axis is roll_axis and the knots sit near the identity (the hypotheses check, which needs every keypoint in view)."""
    rng = np.random.default_rng([28, seed, int(roll)])
    out = []
    for a in ANGLES:
        for sign in (1.0, -1.0):
            i = len(out)
            cap, ex = times(i)
            if roll:
                kt, kR = 0.002 * rng.normal(size=(N_KNOTS, 3)), sign * np.tile([0.0, 0.0, 0.0, 1.0], (N_KNOTS, 1))
                ex = 0.04
                axis = roll_axis(rng)
                ups = _translation(rng) * np.array([1.0, 1.0, 0.3])
            else:
                kt, kR = slow_knots(rng, sign)
                axis = _unit(rng.normal(size=3))
                ups = _translation(rng)
            out.append(dict(angle=a, sign=sign, kt=kt, kR=kR, tan6=np.r_[ups, float(a) * axis], cap=cap, exp=ex, prev=cap - 0.1))
    return out


def log_cases(k, seed=0):
    """Set A of the commit check: per (angle, sign) a pair with zero velocity (the predict leaves its knots bit for bit) whose
    T_prev is built in exact arithmetic so that T_prev^-1 * T(cap) = D, D = (upsilon, sign * quat(axis, angle)), then rounded to
    double.  "pi": every knot is the same rotation (axis, 0) -- the spline's rotation is then that quaternion bit for bit on every
    implementation -- and T_prev's rotation is (0, 0, 0, sign): the product has w == 0 exactly."""
    rng = np.random.default_rng([28, 100 + seed, k])
    out = []
    for a in LOG_ANGLES:
        for sign in (1.0, -1.0):
            i = len(out)
            cap, ex = times(i)
            kt, kR = slow_knots(rng, rng.choice([1.0, -1.0]))
            axis, ups = _unit(rng.normal(size=3)), _translation(rng)
            t0 = cap - 0.5 * ex
            if isinstance(a, str):
                kR = np.tile(np.r_[axis, 0.0], (N_KNOTS, 1))
                T_prev = np.r_[_translation(rng), 0.0, 0.0, 0.0, sign]
            else:
                idx, u = segment(cap, t0, DT)
                p, q = get_pose(k, *knot_lists(kt, kR), idx, u)
                Dq = [D(sign) * v for v in qexp([D(float(a)) * D(x) for x in axis])]
                Dinv = inverse(make(Dq, vec(ups)))
                T_prev = to_float(tmul(make(q, p), Dinv))
            qk = _unit(rng.normal(size=4))
            if a == 0.4:
                # knots 1e-3 off unit length on this one angle: TransformTo's inverse is conjugate / squared norm, and only a
                # quaternion that is not of unit length tells it from the conjugate (the knots of T_prev's construction above are
                # the unit ones: Transformation(q, p) normalises, so the log's argument keeps the case's angle)
                kR = kR * 1.001
            out.append(dict(angle=a, sign=sign, set="A", kt=kt, kR=kR, cap=cap, exp=ex, prev=cap - 0.1, velocity=np.zeros(6), T_prev=T_prev,
                            T_keyframe=np.r_[rng.normal(0, 1, 3), qk]))
    return out


def spline_cases(k, seed=0):
    """Set B of the commit check: ordinary states on roll-dominant splines whose consecutive knots are `angle` apart, both knot signs."""
    rng = np.random.default_rng([28, 200 + seed, k])
    out = []
    for a in ANGLES:
        for flip in (False, True):
            i = len(out)
            cap, ex = times(i)
            kt, kR = 0.002 * rng.normal(size=(N_KNOTS, 3)), roll_knots(rng, float(a), flip)
            vel = np.r_[rng.normal(0, 0.3, 3), rng.normal(0, 0.2, 3)]
            qp, qk = _unit(rng.normal(size=4)), _unit(rng.normal(size=4))
            out.append(dict(angle=a, sign=-1.0 if flip else 1.0, set="B", kt=kt, kR=kR, cap=cap, exp=ex, prev=cap - 0.1, velocity=vel,
                            T_prev=np.r_[rng.normal(0, 0.05, 3), qp], T_keyframe=np.r_[rng.normal(0, 1, 3), qk]))
    return out


def commit_cases(k):
    return log_cases(k) + spline_cases(k)


# the hypotheses check: the call's one twist[1]; hypothesis 0 (velocity * dt_frame alone) then carries 1e3 m sideways
HYP_TWIST = (-1e3, 0.0, 0.0, 0.0, 0.0, 0.0)


def hyp_cases():
    """exp_cases(roll=True) with the stored velocity chosen so that (1 * velocity) * dt_frame + HYP_TWIST is (nearly) the case's
    tangent; `tan1` is that expression in doubles, `tan0` hypothesis 0's."""
    out = exp_cases(roll=True, seed=1)
    for c in out:
        dt_frame = c["cap"] - c["prev"]
        c["velocity"] = (c["tan6"] - np.array(HYP_TWIST)) / dt_frame
        c["tan0"] = np.array(tangent(c["velocity"], dt_frame))
        c["tan1"] = np.array(tangent(c["velocity"], dt_frame, 1.0, HYP_TWIST))
    return out


def fill_states(capi, cases):
    """The B VoState of a list of cases (exp_cases: velocity = tan6 / dt_frame, random unit T_prev / T_keyframe)."""
    rng = np.random.default_rng(2828)
    states = (capi.VoState * len(cases))()
    for c, st in zip(cases, states):
        st.t0, st.dt, st.N, st.is_first = 0.0, DT, N_KNOTS, 0
        st.knots_t[:3 * N_KNOTS] = np.asarray(c["kt"]).ravel().tolist()
        st.knots_R[:4 * N_KNOTS] = np.asarray(c["kR"]).ravel().tolist()
        if "velocity" not in c:
            c["velocity"] = c["tan6"] / (c["cap"] - c["prev"])
        for name in ("T_prev", "T_keyframe"):
            if name not in c:
                c[name] = np.r_[rng.normal(0, 0.05, 3), _unit(rng.normal(size=4))]
        st.T_keyframe[:] = c["T_keyframe"].tolist()
        st.T_prev_b2w[:] = c["T_prev"].tolist()
        st.velocity[:] = np.asarray(c["velocity"]).tolist()
        st.prev_timestamp = float(c["prev"])
    return states


# ---------------------------------------------------------------------------------------------------------------- branches
def exp_branch(tan):
    """Which side of se3_exp's threshold a tangent (doubles) falls: "series" (theta < 1e-10) or "general"."""
    om = [float(v) for v in tan[3:]]
    return "series" if np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]) < 1e-10 else "general"


def log_branch(q):
    """The branch of se3_log / qlog a quaternion (doubles, xyzw) takes, and the side of se3_log's |theta| < 1e-10 test: (branch,
    small_theta) with branch "series" (sn < 1e-20), "pi" (|w| < 1e-10) or "general+" / "general-" by the sign of w."""
    x, y, z, w = (float(v) for v in q)
    sn = x * x + y * y + z * z
    n = np.sqrt(sn)
    if sn < 1e-20:
        two_atan = 2.0 / w - 2.0 * sn / (w * (w * w))
        br = "series"
    elif abs(w) < 1e-10:
        two_atan = (PI_F if w > 0 else -PI_F) / n
        br = "pi"
    else:
        two_atan = 2.0 * np.arctan(n / w) / n
        br = "general+" if w > 0 else "general-"
    return br, abs(two_atan * n) < 1e-10


def named_log_branch(angle):
    """The branch the issue's angle is there for."""
    if isinstance(angle, str) or angle > 3.14:
        return "pi"
    return "series" if angle < 2e-10 else "general"


# ---------------------------------------------------------------------------------------------------------------- errors and bounds
def err(got, want):
    return float(np.abs(np.asarray(got, np.float64).ravel() - np.asarray(want, np.float64).ravel()).max())


def quat_err(got, want):
    """For a result whose quaternion sign is free (exp(log(T)) against T)."""
    return min(err(got, want), err(-np.asarray(got), want))


def floors(cases, host_err):
    """floor[quantity]: the largest host error over the cases with FLOOR_RANGE[0] <= angle <= FLOOR_RANGE[1]."""
    out = {}
    for name, errs in host_err.items():
        vals = [e for c, e in zip(cases, errs) if not isinstance(c["angle"], str) and FLOOR_RANGE[0] <= c["angle"] <= FLOOR_RANGE[1] and e is not None]
        out[name] = max(vals)
    return out


def bounds(cases, host_err):
    """bound[quantity][case] = 4 * max(host_err, floor)."""
    fl = floors(cases, host_err)
    return {name: [None if e is None else 4.0 * max(e, fl[name]) for e in errs] for name, errs in host_err.items()}


def per_angle(cases, values):
    """max over the cases of every angle, in the order of the angle list: [(angle id, value)]."""
    out = {}
    for c, v in zip(cases, values):
        if v is not None:
            key = angle_id(c["angle"])
            out[key] = max(out.get(key, 0.0), v)
    return list(out.items())


# ---------------------------------------------------------------------------------------------------------------- exact and host per check
def predict_exact(cases, key="tan"):
    """[(kt 3N, kR 4N) doubles] of TransformByRight(exp(tangent)) per case; the tangent is c[key] (doubles as the kernel forms them)."""
    out = []
    for c in cases:
        t, R = predict(c["kt"], c["kR"], c[key])
        out.append((to_float([v for r in t for v in r]), to_float([v for r in R for v in r])))
    return out


def predict_host(lib, dp, cases, key="tan"):
    """The same through the C ABI's host algebra: mbavo_se3_exp and mbavo_spline_transform_by_right."""
    out = []
    for c in cases:
        kt, kR = np.array(c["kt"], np.float64).ravel().copy(), np.array(c["kR"], np.float64).ravel().copy()
        dT, tan = np.zeros(7), np.ascontiguousarray(c[key], dtype=np.float64)
        assert lib.mbavo_se3_exp(dp(tan), dp(dT)) == 0
        q, t = np.ascontiguousarray(dT[3:]), np.ascontiguousarray(dT[:3])
        assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), N_KNOTS, dp(q), dp(t)) == 0
        out.append((kt, kR))
    return out


def set_predict_tangents(cases):
    """c["tan"]: velocity * dt_frame in doubles, from the velocity the state holds."""
    for c in cases:
        if "velocity" not in c:
            c["velocity"] = c["tan6"] / (c["cap"] - c["prev"])
        c["tan"] = np.array(tangent(c["velocity"], c["cap"] - c["prev"]))
    return cases


PREDICT_QUANTITIES = ("predict_knots_t", "predict_knots_R")
COMMIT_QUANTITIES = ("T", "velocity", "T_prev", "T_keyframe", "knots_t", "knots_R", "T_world")


def predict_errors(got, exact):
    """{quantity: [error per case]} of (kt, kR) pairs against the exact ones."""
    return dict(predict_knots_t=[err(g[0], e[0]) for g, e in zip(got, exact)], predict_knots_R=[err(g[1], e[1]) for g, e in zip(got, exact)])


def commit_exact(k, cases, verdict):
    """Per case the exact commit (dict of double arrays) after the exact predict, with t0 = cap - exp / 2 as the predict publishes it."""
    out = []
    for c in cases:
        dt_frame = c["cap"] - c["prev"]
        t, R = predict(c["kt"], c["kR"], tangent(c["velocity"], dt_frame))
        t0 = c["cap"] - 0.5 * c["exp"]
        r = commit(k, t, R, t0, DT, c["cap"], c["T_prev"], c["T_keyframe"], dt_frame, verdict)
        d = {name: to_float(v) for name, v in r.items()}
        d["pred_kt"], d["pred_kR"] = to_float([v for r_ in t for v in r_]), to_float([v for r_ in R for v in r_])
        out.append(d)
    return out


def commit_host(lib, dp, k, cases, verdict):
    """The same through the C ABI's host algebra (tests/pairs_track.host_commit's sequence of calls)."""
    out = []
    ident = np.array([0.0, 0, 0, 0, 0, 0, 1])
    for c in cases:
        dt_frame = c["cap"] - c["prev"]
        cc = dict(c, tan=np.array(tangent(c["velocity"], dt_frame)))
        kt, kR = predict_host(lib, dp, [cc])[0]
        t0 = c["cap"] - 0.5 * c["exp"]
        p, q = np.zeros(3), np.zeros(4)
        assert lib.mbavo_spline_get_pose(k, t0, DT, dp(kt), dp(kR), N_KNOTS, float(c["cap"]), dp(p), dp(q), None, None) == 0
        T = np.r_[p, q]
        Tb, Tpi, dTn, lg = np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(6)
        assert lib.mbavo_transform_mul(dp(ident), dp(T), dp(Tb)) == 0  # Transformation(q, p): the normalisation
        Tp, Tk = np.ascontiguousarray(c["T_prev"], dtype=np.float64), np.ascontiguousarray(c["T_keyframe"], dtype=np.float64)
        assert lib.mbavo_transform_inverse(dp(Tp), dp(Tpi)) == 0
        assert lib.mbavo_transform_mul(dp(Tpi), dp(Tb), dp(dTn)) == 0
        assert lib.mbavo_se3_log(dp(dTn), dp(lg)) == 0
        d = dict(T=T, velocity=lg / dt_frame, T_prev=Tb.copy(), T_keyframe=Tk.copy())
        if verdict:
            Tn = np.zeros(7)
            assert lib.mbavo_transform_mul(dp(Tk), dp(Tb), dp(Tn)) == 0
            d["T_keyframe"], d["T_prev"] = Tn, ident.copy()
            qi, ti = np.array([0.0, 0, 0, 1]), np.zeros(3)
            assert lib.mbavo_spline_transform_to(k, t0, DT, dp(kt), dp(kR), N_KNOTS, float(c["cap"]), dp(qi), dp(ti)) == 0
        assert lib.mbavo_spline_get_pose(k, t0, DT, dp(kt), dp(kR), N_KNOTS, float(c["cap"]), dp(p), dp(q), None, None) == 0
        P, Tw = np.zeros(7), np.zeros(7)
        assert lib.mbavo_transform_mul(dp(ident), dp(np.r_[p, q]), dp(P)) == 0
        assert lib.mbavo_transform_mul(dp(d["T_keyframe"]), dp(P), dp(Tw)) == 0
        d.update(knots_t=kt, knots_R=kR, T_world=Tw)
        out.append(d)
    return out


def commit_errors(got, exact):
    return {name: [err(g[name], e[name]) for g, e in zip(got, exact)] for name in COMMIT_QUANTITIES}


def table(title, cases, columns):
    """Text rows "quantity angle col1 col2 ..": columns = [(heading, {quantity: [per case]})]; the maximum per angle."""
    lines = ["%s" % title, "%-16s %-9s %s" % ("quantity", "angle", " ".join("%-11s" % h for h, _ in columns))]
    for name in columns[0][1]:
        cols = [dict(per_angle(cases, col[name])) for _, col in columns]
        for a in cols[0]:
            lines.append("%-16s %-9s %s" % (name, a, " ".join("%-11.3e" % col[a] for col in cols)))
    return "\n".join(lines)
