"""The pairs tracker's pose algebra on the device at EVERY rotation angle, against exact values: k_pairs_predict, k_pairs_commit
(pairs_track.hip) and k_pairs_hypotheses (pairs_hyp.hip) run se3_exp, se3_log and spline_pose with se3_math.h's short fastm forms of
sine, cosine, arctangent, reciprocal and rsqrt; the rest of the suite holds them to the project's own host formulas and only on
rotations between 7e-4 and 0.1 rad (plus 0 and 1e-11).  Here every case is one pair of a batch -- angles from 1e-11 through both
1e-10 thresholds, the 1e-10 .. 1e-4 band where se3_exp's c1 and c2 cancel, every reduction range of the arctangent, 3.1,
pi - 1e-11 and, for the logarithm, exactly pi; both quaternion signs -- and the expectation is tests/pose_algebra_ref.py: 60-digit
decimal arithmetic, the true functions.

Bound, per quantity and case: |device - exact| <= 4 * max(host_err, floor), host_err = |C ABI host algebra - exact| on the same case
and floor the largest host_err of the quantity over the cases with an angle in [1e-2, 2.9]; both computed here on the CPU, nothing
taken from the device (tests/test_pose_algebra_ref.py holds the yardstick itself to the cancellation analysis and to 1e-9 outside the
band).  |device - host| is printed and not asserted; the printed tables are profiles/r28_pose_algebra.txt."""
import numpy as np
import pytest

import pairs_device as dv
import pairs_step as ps
import pairs_track as pt
import pose_algebra_ref as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
# the thresholds that force a verdict on every pair with a keypoint: avg_flow > -1 always, avg_flow > inf never
FORCE = {1: (0.0, -1.0, 0.0), 0: (INF, INF, 0.0)}


def _object(ctx, mbavo, cases, k):
    """A pairs object of len(cases) pairs (one level, 120 x 160, N = 6) prepared on the cases' keypoints, with the cases' states."""
    from mba_vo_amd import synth, workloads
    B = len(cases)
    base = synth.texture_image(ref.H, ref.W, seed=28, octaves=(32, 16, 8, 4))
    other = synth.texture_image(ref.H, ref.W, seed=128, octaves=(32, 16, 8, 4))
    sharp = np.ascontiguousarray(np.stack([np.roll(base, (7 * b, 13 * b), (0, 1)) for b in range(B)]))
    blur = np.ascontiguousarray(np.stack([np.roll(other, (3 * b + 1, 5 * b + 2), (0, 1)) for b in range(B)]))
    pb = workloads.PairBatch(ctx, B, L=1, H=ref.H, W=ref.W, S=8, k=k, N=ref.N_KNOTS, intr=ref.INTR, cell=ps.CELL, thresh=ps.THR, border=4)
    try:
        points = [ref.case_points(b) for b in range(B)]
        counts = pb.prepare_points(*dv.dev(sharp, blur), points)
        assert (counts[:, 0] == ref.K_POINTS).all()
        states = ref.fill_states(mbavo.capi, cases)
        assert pb.set_states(states) == 0
    except Exception:
        pb.close()
        raise
    return pb, points


def _times(cases):
    return np.array([c["cap"] for c in cases]), np.array([c["exp"] for c in cases])


def _hold(title, cases, dev_err, host_err, dev_host):
    """Print host error, device error, device error / bound and |device - host| per quantity and angle; assert the bound per case."""
    b = ref.bounds(cases, host_err)
    ratio = {name: [0.0 if d == 0.0 else (INF if lim == 0.0 else d / lim) for d, lim in zip(dev_err[name], b[name])] for name in dev_err}
    print("\n" + ref.table(title, cases, [("host_err", host_err), ("device_err", dev_err), ("dev/bound", ratio), ("|dev-host|", dev_host)]))
    for name in ("predict_knots_t", "T_prev"):  # pairs_track.MEASURED states the host's bits for these two
        if name in dev_host and pt.MEASURED[name] == 0.0:
            off = [a for a, v in ref.per_angle(cases, dev_host[name]) if v > 0.0]
            print("%s: device and host differ in bits at the angles %s" % (name, ", ".join(off) if off else "(none)"))
    over = [(name, ref.angle_id(c["angle"]), c["sign"], c.get("set", ""), d, lim) for name in dev_err
            for c, d, lim in zip(cases, dev_err[name], b[name]) if not d <= lim]
    assert not over, over


# ---------------------------------------------------------------------------------------------------------------- (a) predict
@pytest.mark.parametrize("k", [2, 4])
def test_predict_at_every_angle(mbavo, gpu_ctx, k):
    lib, dp = gpu_ctx.lib, mbavo.capi.dp
    cases = ref.set_predict_tangents(ref.exp_cases())
    exact, host = ref.predict_exact(cases), ref.predict_host(lib, dp, cases)
    pb, _ = _object(gpu_ctx, mbavo, cases, k)
    try:
        assert pb.predict(*_times(cases)) == 0
        kt, kR = pb.knots()
    finally:
        pb.close()
    dev = [(kt[b].ravel(), kR[b].ravel()) for b in range(len(cases))]
    _hold("predict (k = %d object): TransformByRight(exp(velocity * dt_frame)) against exact values" % k, cases,
          ref.predict_errors(dev, exact), ref.predict_errors(host, exact), ref.predict_errors(dev, host))


# ---------------------------------------------------------------------------------------------------------------- (b) commit
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("verdict", [0, 1])
def test_commit_at_every_angle(orc, mbavo, gpu_ctx, k, verdict):
    """Set A: zero velocity and a T_prev built so that the log's argument has the case's angle and sign.  Set B: ordinary states on
    roll-dominant splines whose knots are the case's angle apart; there the averages are the oracle's as well."""
    lib, dp = gpu_ctx.lib, mbavo.capi.dp
    cases = ref.commit_cases(k)
    exact, host = ref.commit_exact(k, cases, verdict), ref.commit_host(lib, dp, k, cases, verdict)
    pb, points = _object(gpu_ctx, mbavo, cases, k)
    try:
        cap, exp = _times(cases)
        assert pb.predict(cap, exp) == 0
        kt, kR = pb.knots()
        out = pb.commit(*FORCE[verdict])
        after = pb.get_states()
    finally:
        pb.close()
    dev = []
    for b, c in enumerate(cases):
        f = out[b]
        assert f.a.status == 0 and f.a.is_keyframe == verdict and f.a.num_keypoints0 == ref.K_POINTS, b
        got = pt.state_arrays(after[b])
        dev.append(dict(T=np.array(f.a.T), velocity=got["velocity"], T_prev=got["T_prev"], T_keyframe=got["T_keyframe"], knots_t=got["kt"],
                        knots_R=got["kR"], T_world=np.array(f.T_world)))
        assert got["prev_timestamp"] == c["cap"] and got["t0"] == c["cap"] - 0.5 * c["exp"]
        if c["set"] == "A":  # exp(0) is the identity bit for bit: the log's argument is what the case builder made
            assert np.array_equal(kt[b], c["kt"]) and np.array_equal(kR[b], c["kR"]), b
        else:
            xy, z = points[b]
            v, af, ak = ps.oracle_assess(orc, ref.INTR, xy, z, k, c["cap"] - 0.5 * c["exp"], ref.DT, exact[b]["pred_kt"], exact[b]["pred_kR"],
                                         c["cap"], c["exp"], FORCE[verdict])
            assert v == verdict and abs(f.a.avg_flow - af) <= ps.bound(af) and abs(f.a.avg_kernel - ak) <= ps.bound(ak), \
                (b, ref.angle_id(c["angle"]), f.a.avg_flow, af, f.a.avg_kernel, ak)
        if not verdict:
            assert np.array_equal(got["kt"], kt[b].ravel()) and np.array_equal(got["kR"], kR[b].ravel()), b
    _hold("commit k = %d verdict %d: log at the angle (set A), spline knots the angle apart (set B), against exact values" % (k, verdict),
          cases, ref.commit_errors(dev, exact), ref.commit_errors(host, exact), ref.commit_errors(dev, host))


# ---------------------------------------------------------------------------------------------------------------- (c) hypotheses
@pytest.mark.parametrize("k", [2, 4])
def test_hypothesis_knots_at_every_angle(mbavo, gpu_ctx, k):
    """M = 2: hypothesis 0 carries every keypoint 1e3 m out of view, hypothesis 1 = (1 * velocity) * dt_frame + twist is the case's
    roll-dominant tangent (tests/test_pose_algebra_ref.py asserts both on the CPU), so the knots left behind are candidate 1's."""
    lib, dp = gpu_ctx.lib, mbavo.capi.dp
    cases = ref.hyp_cases()
    exact, host = ref.predict_exact(cases, "tan1"), ref.predict_host(lib, dp, cases, "tan1")
    pb, _ = _object(gpu_ctx, mbavo, cases, k)
    try:
        rc, rec = pb.predict_hypotheses(*_times(cases), [1.0], [ref.HYP_TWIST], level=0, min_valid_frac=0.5)
        assert rc == 0
        kt, kR = pb.knots()
    finally:
        pb.close()
    for b, r in enumerate(rec):
        assert (r.winner, r.num_eligible, r.status, r.num_keypoints) == (1, 1, 0, ref.K_POINTS) and r.valid[0] == 0.0, \
            (b, r.winner, r.num_eligible, r.status, r.valid[0], r.valid[1])
    dev = [(kt[b].ravel(), kR[b].ravel()) for b in range(len(cases))]
    _hold("hypotheses k = %d: TransformByRight(exp((1 * velocity) * dt_frame + twist)) against exact values" % k, cases,
          ref.predict_errors(dev, exact), ref.predict_errors(host, exact), ref.predict_errors(dev, host))
