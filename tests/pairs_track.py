"""Shared by tests/test_pairs_track_api.py (CPU) and tests/test_gpu_pairs_track.py (GPU): trackFrame's pose bookkeeping
(blur_aware_direct_tracker.cpp:119-141 and :150-188) restated on the host with the C ABI's own algebra -- mbavo_se3_exp / _log,
mbavo_transform_mul / _inverse, mbavo_spline_transform_by_right / _to, mbavo_spline_get_pose -- the states the GPU checks start
from, and the bounds they hold the device to.

Algebra bound.  mbavo_pairs_predict and mbavo_pairs_commit do the same operations as the host restatement; what differs is the
device's sine / cosine / arctangent (fdlibm kernels, a few units in the last place from libm's) and possible contraction inside
the spline sample.  The bound per quantity is 4 x the largest absolute difference seen on the first GPU run over all cases of
checks 1 and 2 (MEASURED below, also in profiles/r12_pairs_track.txt), and never more than ALGEBRA_CAP = 1e-9: the cap is a
condition, not a measurement -- a wrong formula (a dropped V(omega), a swapped product, TransformTo with the un-normalised
inverse) shows at >= 1e-5 on these motions."""
import ctypes as C

import numpy as np

import pairs_step as ps

ALGEBRA_CAP = 1e-9
# largest |device - host restatement| per quantity over ASSESS_CASES (first GPU run; the test prints them on every run).  A zero is a
# quantity that came out with the host's bits on every pair of every case: its bound asks for that again.
# To re-measure (a new ROCm or libm may move the last bits of sin / cos / atan on either side, with the code still right): run
# `python -m pytest -m gpu -s tests/test_gpu_pairs_track.py -k host_algebra`, take the last "algebra maxima so far" line, put its
# figures here and into the "measured bounds" section of profiles/r12_pairs_track.txt.  A figure that no longer fits under
# ALGEBRA_CAP / 4 is a defect, not a new figure.
MEASURED = dict(predict_knots_t=0.0, predict_knots_R=6.939e-18, velocity=7.105e-15, T_prev=0.0, T_keyframe=2.220e-16, knots_t=1.110e-16,
                knots_R=8.674e-19, T_world=2.220e-16)


def algebra_bound(name):
    b = 4.0 * MEASURED[name]
    assert b <= ALGEBRA_CAP, (name, b)
    return b


def random_pose(rng, scale=1.0):
    q = rng.normal(0, 1, 4)
    return np.r_[rng.normal(0, scale, 3), q / np.linalg.norm(q)]


def make_states(capi, case, seed=0):
    """B tracker states on the knots of an assess case (tests/pairs_step.assess_inputs): random unit-quaternion T_keyframe and
    T_prev_b2w, a velocity scaled per pair by pairs_step.SCALES -- pair 1 with zero velocity and pair 2 with |omega| < 1e-10 (the
    small-angle branches of exp; B = 1: the plain case only) -- and the previous frame 0.1 s before the capture time."""
    rng = np.random.default_rng(1000 + seed)
    B, N = case["B"], case["kt"].shape[1]
    states = (capi.VoState * B)()
    for b, st in enumerate(states):
        st.t0, st.dt, st.N, st.is_first = float(case["t0"][b]), float(case["dt"]), N, 0
        st.knots_t[:3 * N] = case["kt"][b].ravel().tolist()
        st.knots_R[:4 * N] = case["kR"][b].ravel().tolist()
        st.T_keyframe[:] = random_pose(rng).tolist()
        st.T_prev_b2w[:] = random_pose(rng, 0.05).tolist()
        s = ps.SCALES[b % len(ps.SCALES)]
        vel = np.r_[rng.normal(0, 0.3, 3), rng.normal(0, 0.2, 3)] * s
        if b == 1:
            vel[:] = 0.0
        if b == 2:
            vel[3:] *= 1e-11 / np.linalg.norm(vel[3:]) / 0.1
        st.velocity[:] = vel.tolist()
        st.prev_timestamp = float(case["cap"][b]) - 0.1
    return states


def copy_state(capi, st):
    out = capi.VoState()
    C.memmove(C.byref(out), C.byref(st), C.sizeof(out))
    return out


def normalized_pose(T):
    """Core::Transformation(q, t) of a GetPose result: Eigen normalized() in the host code's own order of operations (Python
    floats are IEEE doubles: the same bits)."""
    x, y, z, w = (float(v) for v in T[3:])
    n2 = x * x + y * y + z * z + w * w
    n = np.sqrt(n2) if n2 > 0 else 1.0
    return np.array([T[0], T[1], T[2], x / n, y / n, z / n, w / n])


def host_predict(lib, dp, st, cap, exp):
    """:119-141 on one state: (t0, knots_t 3N, knots_R 4N, dt_frame)."""
    return ps.predict(lib, dp, st, cap, exp)


def host_commit(lib, dp, k, st, t0, kt, kR, dt_frame, T, verdict, cap):
    """:150-188 and the output pose on one pair with the C ABI's algebra.  st: the state before the frame (T_keyframe, T_prev_b2w);
    t0, kt, kR: the spline after the alignment; T: its pose at the capture time (7 doubles, as GetPose returns it).
    Returns dict(velocity, T_prev, T_keyframe, kt, kR, T_world)."""
    N = st.N
    kt, kR = np.array(kt, dtype=np.float64).ravel().copy(), np.array(kR, dtype=np.float64).ravel().copy()
    T = np.ascontiguousarray(T, dtype=np.float64)
    Tk, Tp = np.array(st.T_keyframe), np.array(st.T_prev_b2w)
    Tpi, dTn, lg, Tb = np.zeros(7), np.zeros(7), np.zeros(6), np.zeros(7)
    ident = np.array([0.0, 0, 0, 0, 0, 0, 1])
    Tb[:] = normalized_pose(T)
    assert lib.mbavo_transform_inverse(dp(Tp), dp(Tpi)) == 0
    assert lib.mbavo_transform_mul(dp(Tpi), dp(Tb), dp(dTn)) == 0
    assert lib.mbavo_se3_log(dp(dTn), dp(lg)) == 0
    out = dict(velocity=lg / dt_frame, T_prev=Tb.copy(), T_keyframe=Tk.copy())
    if verdict:
        Tn = np.zeros(7)
        assert lib.mbavo_transform_mul(dp(Tk), dp(Tb), dp(Tn)) == 0
        out["T_keyframe"] = Tn
        qi, ti = np.array([0.0, 0, 0, 1]), np.zeros(3)
        assert lib.mbavo_spline_transform_to(k, float(t0), float(st.dt), dp(kt), dp(kR), N, float(cap), dp(qi), dp(ti)) == 0
        out["T_prev"] = ident.copy()
    p, q = np.zeros(3), np.zeros(4)
    assert lib.mbavo_spline_get_pose(k, float(t0), float(st.dt), dp(kt), dp(kR), N, float(cap), dp(p), dp(q), None, None) == 0
    Tw = np.zeros(7)
    assert lib.mbavo_transform_mul(dp(out["T_keyframe"]), dp(np.r_[p, q]), dp(Tw)) == 0
    out.update(kt=kt, kR=kR, T_world=Tw)
    return out


def state_arrays(st):
    N = st.N
    return dict(kt=np.array(st.knots_t[:3 * N]), kR=np.array(st.knots_R[:4 * N]), T_keyframe=np.array(st.T_keyframe),
                T_prev=np.array(st.T_prev_b2w), velocity=np.array(st.velocity), prev_timestamp=st.prev_timestamp, t0=st.t0, dt=st.dt)


def states_bytes(states):
    return bytes(states)


# ---- the free-running batch (check 8): T_world at frame i within i * KNOT_TOL of the free-running mbavo_vo tracker's -- the
# project's per-frame tolerance between the device LM and the host LM (tests/test_gpu_lm_batch_levels._check_against), taken to
# accumulate linearly over the frames a state has been carried.
def free_running_bound(i):
    return i * ps.KNOT_TOL


def keyframe_margins(out, thresholds=(ps.FLOW0, ps.FLOW1, ps.KERNEL)):
    """Smallest distance of avg_flow / avg_kernel from the thresholds they are compared with, over one tracker run's frames >= 1."""
    m = np.inf
    for o in out[1:]:
        m = min(m, abs(o["avg_flow"] - thresholds[0]), abs(o["avg_flow"] - thresholds[1]), abs(o["avg_kernel"] - thresholds[2]))
    return m
