"""The exact reference of the tracker's pose algebra (tests/pose_algebra_ref.py) against itself, the C ABI's HOST algebra against it
on every case of tests/test_gpu_pairs_pose_angles.py -- the yardstick that file's bounds are made of -- and the preconditions of its
cases.  No GPU.

What the cancellation analysis predicts for the host's se3_exp (pose_math.h, the reference's formula): V = I + c1 hat + c2 hat^2
with c1 = (1 - cos th) / th^2.  An absolute error of eps / 2 in cos th (one rounding of a number next to 1) is an error of
eps / (2 th^2) in c1 and of eps / (2 th) * |upsilon| in the translation; where cos th rounds to 1 the error is th / 2 * |upsilon|
instead, and below th = 1e-10 the code's V = R is th / 2 * |upsilon| from V as well.  So the translation of exp is held to
    min(EPS / th, th) * |upsilon|   +   a few ulp
for th < 1e-3 (EPS = 2^-52: twice the one-rounding figure, for the second rounding in 1 - cos), and to a few ulp from 1e-3 up.  The
logarithm has no such band: its c2 multiplies hat^2 ~ th^2, which cancels the th^-2."""
import numpy as np
import pytest

import pose_algebra_ref as ref
from pose_algebra_ref import D, Dec

EPS = 2.0 ** -52
ULPS = 16 * EPS  # "a few ulp" of quantities of size <= 2: products of three or four rounded factors, sums of a dozen terms


@pytest.fixture(scope="module")
def host(mbavo):
    return mbavo.load(), mbavo.capi.dp


# ---------------------------------------------------------------------------------------------------------------- (a) the reference
def _rand_tangents():
    rng = np.random.default_rng(5)
    for a in ref.ANGLES:
        for _ in range(2):
            ax = rng.normal(size=3)
            yield a, np.r_[ref._translation(rng), float(a) * ax / np.linalg.norm(ax)]


def test_log_of_exp_and_exp_of_log():
    tol = Dec(10) ** -40
    for a, x in _rand_tangents():
        xs = ref.vec(x)
        T = ref.se3_exp(xs)
        back = ref.se3_log(T)
        assert max(abs(u - v) for u, v in zip(back, xs)) < tol, (a, back, xs)
        again = ref.se3_exp(back)
        assert max(abs(u - v) for u, v in zip(again, T)) < tol, a
        # the other quaternion sign: the logarithm's convention returns the same tangent (theta = 2 atan(n / w) changes sign with w
        # and so does the vector part), and exp gives the rotation back with the quaternion the convention prefers (w > 0)
        neg = T[:3] + [-v for v in T[3:]]
        assert max(abs(u - v) for u, v in zip(ref.se3_log(neg), xs)) < tol, a
    # w == 0: theta = -pi about the quaternion's own axis
    ax = np.array([0.6, 0.0, 0.8])
    lg = ref.se3_log(ref.vec(np.r_[0.1, 0.2, 0.3, ax, 0.0]))
    assert max(abs(u + ref.PI * D(v)) for u, v in zip(lg[3:], ax)) < Dec(10) ** -15  # (0.6, 0.8 are not exact: |axis| - 1 ~ 1e-17)
    T = ref.se3_exp(lg)
    assert max(abs(u + v) for u, v in zip(T[3:6], ref.vec(ax))) < Dec(10) ** -15 and abs(T[6]) < Dec(10) ** -50


def test_inverse_and_product():
    rng = np.random.default_rng(6)
    tol = Dec(10) ** -40
    for _ in range(20):
        q = rng.normal(size=4)
        T = ref.make(ref.vec(q), ref.vec(rng.normal(size=3)))
        for P in (ref.tmul(T, ref.inverse(T)), ref.tmul(ref.inverse(T), T)):
            assert max(abs(u - v) for u, v in zip(P, ref.IDENTITY)) < tol
        U = ref.make(ref.vec(rng.normal(size=4)), ref.vec(rng.normal(size=3)))
        a, b = ref.inverse(ref.tmul(T, U)), ref.tmul(ref.inverse(U), ref.inverse(T))
        assert max(abs(u - v) for u, v in zip(a, b)) < tol
        # a rotated point: q p q^-1 keeps the length
        p = ref.vec(rng.normal(size=3))
        assert abs(ref.norm2(ref.qrot(T[3:], p)) - ref.norm2(p)) < tol


@pytest.mark.parametrize("k", [2, 4])
def test_spline_at_u_zero_is_the_blend_of_the_definition(k):
    """u = 0.  k = 2: knot 0 itself.  k = 4: p = (t0 + 4 t1 + t2) / 6 and q = R0 exp(5/6 log(R0^-1 R1)) exp(1/6 log(R1^-1 R2)); on
    knots a constant rotation apart about one axis that is R0 * rot(axis, (5/6 + 1/6) angle) = R1."""
    rng = np.random.default_rng(7)
    tol = Dec(10) ** -40
    for angle in (1e-9, 0.3, 2.9):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        d = ref.qexp([D(angle) * D(v) for v in axis])
        R = [ref.make(ref.vec(rng.normal(size=4)), [ref.ZERO] * 3)[3:]]
        for _ in range(k - 1):
            R.append(ref.qmul(R[-1], d))
        t = [ref.vec(rng.normal(size=3)) for _ in range(k)]
        p, q = ref.get_pose(k, t, R, 0, 0.0)
        if k == 2:
            want_p, want_q = t[0], R[0]
        else:
            want_p, want_q = [(t[0][a] + 4 * t[1][a] + t[2][a]) / 6 for a in range(3)], R[1]
        assert max(abs(u - v) for u, v in zip(p, want_p)) < tol and max(abs(u - v) for u, v in zip(q, want_q)) < tol, (k, angle)
        # and the end of the segment is the start of the next one's blend: u = 1 on knots 0 .. k-1 equals u = 0 on knots 1 .. k
        if k == 4:
            R.append(ref.qmul(R[-1], d))
            t.append(ref.vec(rng.normal(size=3)))
            p1, q1 = ref.get_pose(4, t, R, 0, 1.0)
            p0, q0 = ref.get_pose(4, t, R, 1, 0.0)
            assert max(abs(u - v) for u, v in zip(p1 + q1, p0 + q0)) < tol


def test_sine_cosine_arctangent_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    args = set()
    for a in ref.ANGLES:
        args.update([float(a), 0.5 * float(a), 0.04 * float(a), -float(a)])
    rel = Dec(10) ** -45
    for x in sorted(args):
        s, c = ref.sincos(D(x))
        ms, mc = mp.sin(mp.mpf(x)), mp.cos(mp.mpf(x))
        assert abs(s - Dec(mp.nstr(ms, 75))) <= rel * abs(s) and abs(c - Dec(mp.nstr(mc, 75))) <= rel, x
    ratios = [np.tan(0.5 * float(a)) for a in ref.ANGLES] + [0.4375, 0.6875, 1.1875, 2.4375, 1e15, -3.0, 1.0]
    for x in ratios:
        got, want = ref.atan(D(x)), Dec(mp.nstr(mp.atan(mp.mpf(float(x))), 75))
        assert abs(got - want) <= rel * abs(want), x
    assert abs(ref.PI - Dec(mp.nstr(mp.pi, 75))) < Dec(10) ** -55


# ---------------------------------------------------------------------------------------------------------------- (b) the host algebra
def _exp_shape(c):
    """The bound the analysis gives the translation of exp(c's tangent)."""
    th = float(np.linalg.norm(c["tan"][3:]))
    ups = float(np.linalg.norm(c["tan"][:3]))
    return (min(EPS / th, th) * ups if th < ref.BAND[1] else 0.0) + ULPS


def test_host_exp_and_log_have_the_predicted_shape(host):
    """mbavo_se3_exp and mbavo_se3_log alone, on the tangents and poses of the cases."""
    lib, dp = host
    rows = []
    for c in ref.set_predict_tangents(ref.exp_cases()):
        T = np.zeros(7)
        assert lib.mbavo_se3_exp(dp(np.ascontiguousarray(c["tan"])), dp(T)) == 0
        want = ref.to_float(ref.se3_exp(ref.vec(c["tan"])))
        et, eq = ref.err(T[:3], want[:3]), ref.err(T[3:], want[3:])
        rows.append((c["angle"], et, eq))
        assert et <= _exp_shape(c), (ref.angle_id(c["angle"]), et, _exp_shape(c))
        assert eq <= ULPS, (ref.angle_id(c["angle"]), eq)
    print("\nhost mbavo_se3_exp against the exact exponential: angle, max |t error|, max |q error|")
    for a in ref.ANGLES:
        sel = [r for r in rows if r[0] == a]
        print("  %-9s %.3e %.3e" % (ref.angle_id(a), max(r[1] for r in sel), max(r[2] for r in sel)))
    rng = np.random.default_rng(9)
    print("host mbavo_se3_log against the exact logarithm: angle, max |upsilon error|, max |omega error|")
    for a in ref.LOG_ANGLES:
        worst = [0.0, 0.0]
        for sign in (1.0, -1.0):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            q = np.r_[ax, 0.0] if isinstance(a, str) else np.r_[np.sin(0.5 * a) * ax, np.cos(0.5 * a)]
            T = np.r_[ref._translation(rng), sign * q]
            T[3:] /= np.sqrt((T[3:] * T[3:]).sum())
            lg = np.zeros(6)
            assert lib.mbavo_se3_log(dp(T), dp(lg)) == 0
            want = ref.to_float(ref.se3_log(ref.vec(T)))
            worst = [max(worst[0], ref.err(lg[:3], want[:3])), max(worst[1], ref.err(lg[3:], want[3:]))]
        print("  %-9s %.3e %.3e" % (ref.angle_id(a), worst[0], worst[1]))
        # pi - 1e-11 takes the |w| < 1e-10 branch, which returns pi: 1e-11 from the true angle.  Everything else: a few ulp of pi
        lim = 1.01e-11 if a == ref.ANGLES[-1] else ULPS
        assert worst[0] <= lim and worst[1] <= lim, (ref.angle_id(a), worst)


def _report(title, cases, host_err):
    b = ref.bounds(cases, host_err)
    print("\n" + ref.table(title, cases, [("host_err", host_err), ("bound", b)]))
    print("floors: %s" % "  ".join("%s %.3e" % kv for kv in ref.floors(cases, host_err).items()))
    for name, bs in b.items():
        for c, v in zip(cases, bs):
            if ref.angle_value(c["angle"]) >= ref.BAND[1]:
                assert v <= ref.ALGEBRA_CAP, (name, ref.angle_id(c["angle"]), v)
    return b


def test_host_predict_yardstick(host):
    """host_err of the predict check and of the hypotheses check, the bounds they give, and the cap outside the band."""
    lib, dp = host
    cases = ref.set_predict_tangents(ref.exp_cases())
    he = ref.predict_errors(ref.predict_host(lib, dp, cases), ref.predict_exact(cases))
    _report("predict: TransformByRight(exp(velocity * dt_frame))", cases, he)
    for c, e in zip(cases, he["predict_knots_t"]):
        assert e <= 2.0 * _exp_shape(c), (ref.angle_id(c["angle"]), e)  # (|R_i| = 1: the knot carries exp's translation error)
    for e in he["predict_knots_R"]:
        assert e <= ULPS
    hyp = ref.hyp_cases()
    hh = ref.predict_errors(ref.predict_host(lib, dp, hyp, "tan1"), ref.predict_exact(hyp, "tan1"))
    _report("hypotheses: TransformByRight(exp((1 * velocity) * dt_frame + twist))", hyp, hh)
    for c, e in zip(hyp, hh["predict_knots_t"]):
        assert e <= 2.0 * _exp_shape(dict(c, tan=c["tan1"])), (ref.angle_id(c["angle"]), e)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("verdict", [0, 1])
def test_host_commit_yardstick(host, k, verdict):
    lib, dp = host
    cases = ref.commit_cases(k)
    he = ref.commit_errors(ref.commit_host(lib, dp, k, cases, verdict), ref.commit_exact(k, cases, verdict))
    _report("commit k = %d verdict %d: sets A (log at the angle) and B (spline knots the angle apart)" % (k, verdict), cases, he)
    for name, errs in he.items():
        for c, e in zip(cases, errs):
            a, scale = ref.angle_value(c["angle"]), 1.0 / (c["cap"] - c["prev"]) if name == "velocity" else 1.0
            # what a threshold of the host's formula costs: pi - 1e-11 is returned as pi (the log of set A, qlog of set B)
            # -- once in set A, once per segment in set B, weighted with the cumulative basis: u <= 1 (k = 2), c1 + c2 + c3 <= 2.17
            # (k = 4).  Neither set has a band: A's predict is the identity, B's runs exp at an ordinary angle.
            segs = 2.2 if (c["set"] == "B" and k == 4) else 1.0
            lim = (1.01e-11 * segs if c["angle"] == ref.ANGLES[-1] else 0.0) + 4 * ULPS
            assert e <= lim * scale, (name, c["set"], ref.angle_id(c["angle"]), e, lim * scale)


# ---------------------------------------------------------------------------------------------------------------- (c) preconditions
def test_exp_cases_sit_on_both_sides_of_the_threshold():
    for cases, key in ((ref.set_predict_tangents(ref.exp_cases()), "tan"), (ref.hyp_cases(), "tan1")):
        got = {ref.angle_id(c["angle"]): ref.exp_branch(c[key]) for c in cases}
        assert got["1e-11"] == got["9.9e-11"] == "series" and got["1.01e-10"] == got["1e-09"] == "general", got
        assert {c["sign"] for c in cases} == {1.0, -1.0}
        for c in cases:
            th = np.linalg.norm(c[key][3:])
            assert abs(th - c["angle"]) <= 1e-6 * c["angle"] and 0.03 * 0.3 <= np.linalg.norm(c["tan6"][:3]) <= 0.3


@pytest.mark.parametrize("k", [2, 4])
def test_log_cases_land_in_their_branches(k):
    """Set A: the quaternion of T_prev^-1 * T(cap), formed in doubles as the kernel forms it, takes the branch the angle is there for
    with the case's sign of w; exactly pi has w == 0.  Set B: every relative quaternion of the (predicted) knots likewise."""
    seen, small = set(), set()
    for c in ref.log_cases(k):
        idx, u = ref.segment(c["cap"], c["cap"] - 0.5 * c["exp"], ref.DT)
        assert idx == 0 and 0 < u < 1
        p, q = ref.get_pose(k, *ref.knot_lists(c["kt"], c["kR"]), idx, u)
        Tb = ref.to_float(ref.make(q, p))
        Ti = ref.to_float(ref.inverse(ref.vec(c["T_prev"])))
        qd = ref._np_qmul(Ti[3:], Tb[3:])
        br, sm = ref.log_branch(qd)
        want = ref.named_log_branch(c["angle"])
        assert br.rstrip("+-") == want, (ref.angle_id(c["angle"]), br, want)
        if isinstance(c["angle"], str):
            assert qd[3] == 0.0
        else:
            assert np.sign(qd[3]) == c["sign"], (ref.angle_id(c["angle"]), qd[3])
            assert sm == (c["angle"] < 1e-10)
            exact = ref.to_float(ref.se3_log(ref.tmul(ref.inverse(ref.vec(c["T_prev"])), ref.make(q, p))))
            assert abs(np.linalg.norm(exact[3:]) - c["angle"]) <= 1e-4 * c["angle"] + 1e-15  # (T_prev is rounded: ~1e-16 of angle)
        seen.add((br, np.sign(qd[3])))
        small.add(sm)
    assert seen >= {("series", 1.0), ("series", -1.0), ("general+", 1.0), ("general-", -1.0), ("pi", 1.0), ("pi", -1.0), ("pi", 0.0)}, seen
    assert small == {True, False}
    seen = set()
    for c in ref.spline_cases(k):
        R = ref.predict_exact([dict(c, tan=ref.tangent(c["velocity"], c["cap"] - c["prev"]))])[0][1].reshape(-1, 4)
        for a, b in zip(R[:k - 1], R[1:k]):
            rel = ref._np_qmul(np.r_[-a[:3], a[3]], b)
            br, _ = ref.log_branch(rel)
            assert br.rstrip("+-") == ref.named_log_branch(c["angle"]), (ref.angle_id(c["angle"]), br)
            # the exact product has the same sign of w: the reference and the kernel take the same side of the cut at +-pi
            ex = ref.qmul(ref.qconj(ref.vec(a)), ref.vec(b))[3]
            assert (ex > 0) == (rel[3] > 0) and abs(float(ex)) > 1e-13
            seen.add((br, bool(rel[3] > 0)))
    assert seen >= {("series", True), ("series", False), ("general+", True), ("general-", False), ("pi", True), ("pi", False)}, seen


def _project(T, xy, z):
    fx, fy, cx, cy = ref.INTR
    x, y, zq, w = T[3:] / np.linalg.norm(T[3:])
    R = np.array([[1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w)],
                  [2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w)],
                  [2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)]])
    P = np.stack([(xy[:, 0] - cx) / fx * z, (xy[:, 1] - cy) / fy * z, z], 1)
    Pc = (P - T[:3]) @ R
    return np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1), Pc[:, 2]


@pytest.mark.parametrize("k", [2, 4])
def test_hypotheses_cases_keep_their_keypoints_in_view(k):
    """Under hypothesis 1 every keypoint of every pair projects at least 8 px inside the image at the capture time and at both
    ends of the exposure (the 8-pixel pattern reaches 2 px); under hypothesis 0 none projects inside it."""
    cases = ref.hyp_cases()
    for key, inside in (("tan1", True), ("tan0", False)):
        knots = ref.predict_exact(cases, key)
        for i, (c, (kt, kR)) in enumerate(zip(cases, knots)):
            xy, z = ref.case_points(i)
            t0 = c["cap"] - 0.5 * c["exp"]
            for t in (c["cap"], c["cap"] - 0.5 * c["exp"], c["cap"] + 0.5 * c["exp"]):
                idx, u = ref.segment(t, t0, ref.DT)
                p, q = ref.get_pose(k, *ref.knot_lists(kt, kR), idx, u)
                px, depth = _project(ref.to_float(p + q), xy, z)
                ok = (px[:, 0] >= 8) & (px[:, 0] <= ref.W - 9) & (px[:, 1] >= 8) & (px[:, 1] <= ref.H - 9) & (depth > 0.5)
                if inside:
                    assert ok.all(), (ref.angle_id(c["angle"]), px[~ok])
                else:
                    out = (px[:, 0] < -8) | (px[:, 0] > ref.W + 8) | (px[:, 1] < -8) | (px[:, 1] > ref.H + 8) | (depth < 0)
                    assert out.all(), ref.angle_id(c["angle"])
