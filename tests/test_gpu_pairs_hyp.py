"""mbavo_pairs_predict_hypotheses on the device, through the C ABI: every pair's start picked among M motion hypotheses, in
predict's place.  Held to mbavo_pairs_predict bit for bit where the two must agree (M = 1, winner 0), to the ORACLE run on the
entry rebuilt from the object's own device arrays (tests/pairs_oracle.read_entry) with the restated candidate knots
(tests/pairs_hyp_ref.py) for every score and valid count, and to the restated selection rule for every winner.

Bounds: valid counts exact; scores 1e-9 relative, what tests/test_gpu_pairs_oracle.py holds the cost to; the winner's knots within
pairs_track.algebra_bound("predict_knots_*") of the host algebra's candidate.  The preconditions of the winner checks (scores
separated by more than 1 %, the flung-out hypothesis without a pixel) are asserted on the CPU by tests/test_pairs_hyp_api.py on the
same inputs."""
import ctypes as C

import numpy as np
import pytest

import pairs_device as dv
import pairs_hyp_ref as hr
import pairs_hyp_support as hs
import pairs_oracle as po
import pairs_step as ps
import pairs_track as pt

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -2
THRESHOLDS = (ps.FLOW0, ps.FLOW1, ps.KERNEL)
L = hr.LEVELS


def _batch(ctx, case, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, case["B"], L=L, H=case["H"], W=case["W"], S=hr.S, k=case["k"], N=ps.N_KNOTS, cell=ps.CELL, thresh=ps.THR,
                               border=hr.BORDER, huber=hr.HUBER, **kw)


def _prepared(ctx, case, states, **kw):
    pb = _batch(ctx, case, **kw)
    try:
        pb.prepare(*dv.dev(case["sharp"], case["depth"], case["blur"]))
        assert pb.set_states(states) == 0
    except Exception:
        pb.close()
        raise
    return pb


def _problem_times(pb):
    return [(pb.array[e].t0, pb.array[e].dt, pb.array[e].h_start_idx[0]) for e in range(pb.B * pb.L)]


def _knot_bytes(pb):
    kt, kR = pb.knots()
    return kt.tobytes() + kR.tobytes()


def _snapshot(pb):
    return _knot_bytes(pb), bytes(pb.get_states()), _problem_times(pb)


def _assess_case(capi, B, H, W, k):
    case = ps.assess_inputs(B, H, W, k)
    return case, pt.make_states(capi, case)


_launches_of_last_evaluation = hs.launches_of_last_evaluation


def _mixed(M, seed):
    """M - 1 scales and twists of every kind: zero, negative and large scales, twists in v, in w, in both, and none."""
    rng = np.random.default_rng(seed)
    scales = rng.uniform(-1.5, 2.5, M - 1)
    scales[0] = 0.0
    twists = [np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.02, 3)] for _ in range(M - 1)]
    twists[0] = None
    if M > 2:
        twists[1][:3] = 0.0
    if M > 3:
        twists[2][3:] = 0.0
    return scales.tolist(), twists


# ---- 1. M = 1 is predict
@pytest.mark.parametrize("B,H,W,k", hr.WIN_CASES)
def test_one_hypothesis_is_predict(mbavo, gpu_ctx, B, H, W, k):
    case, states = _assess_case(mbavo.capi, B, H, W, k)
    pb, twin = _prepared(gpu_ctx, case, states), _prepared(gpu_ctx, case, states)
    try:
        rc, rec = pb.predict_hypotheses(case["cap"], case["exp"], [], [], level=1)
        assert rc == 0 and twin.predict(case["cap"], case["exp"]) == 0
        assert all(r.winner == 0 and r.num_eligible in (0, 1) for r in rec)
        a, b = _snapshot(pb), _snapshot(twin)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert pb.knots()[0].tobytes() != case["kt"].tobytes()  # (something moved)
        assert bytes(pb.commit(*THRESHOLDS)) == bytes(twin.commit(*THRESHOLDS))
        assert _snapshot(pb) == _snapshot(twin)
    finally:
        pb.close()
        twin.close()


# ---- 2. scores and valid counts against the oracle on rebuilt entries
def _check_scores(orc, mbavo, ctx, pb, states, cap, exp, scales, twists, level, tag, min_valid_frac=0, min_gain=0):
    """tests/pairs_hyp_support.check_scores: the oracle on the rebuilt entries, the selection rule on the device's own numbers."""
    opts = dict(scales=scales, twists=twists, level=level, min_valid_frac=min_valid_frac, min_gain=min_gain)
    return hs.check_scores(orc, mbavo, ctx, pb, states, cap, exp, opts, tag)


@pytest.mark.parametrize("B,H,W,k", hr.WIN_CASES)
@pytest.mark.parametrize("M,level", [(4, 0), (16, L - 1)])
def test_scores_match_the_oracle_on_rebuilt_entries(orc, mbavo, gpu_ctx, B, H, W, k, M, level):
    case, states = _assess_case(mbavo.capi, B, H, W, k)
    pb = _prepared(gpu_ctx, case, states)
    try:
        scales, twists = _mixed(M, 10 * M + B)
        _check_scores(orc, mbavo, gpu_ctx, pb, states, case["cap"], case["exp"], scales, twists, level, (B, k, M, level))
    finally:
        pb.close()


# ---- 3. the winner and its knots; 5. min_gain
@pytest.mark.parametrize("B,H,W,k", hr.WIN_CASES)
def test_winner_is_the_oracles_and_the_lm_starts_from_it(orc, mbavo, gpu_ctx, B, H, W, k):
    import torch
    capi = mbavo.capi
    case = hr.win_case(orc, mbavo, B, H, W, k)
    states, cap, exp = case["states"], case["cap"], case["exp"]
    pb, twin = _prepared(gpu_ctx, case, states), _prepared(gpu_ctx, case, states)
    level = L - 1
    try:
        rec, oracle, cands = _check_scores(orc, mbavo, gpu_ctx, pb, states, cap, exp, hr.WIN_SCALES, hr.WIN_TWISTS, level, ("winner", B, k))
        assert twin.predict(cap, exp) == 0
        kt, kR = pb.knots()
        tkt, tkR = twin.knots()
        for b in range(B):
            scores, valids, elig, costs = oracle[b]
            w = hr.winner(scores, elig)[0]
            assert rec[b].winner == w == case["truth"][b], (b, rec[b].winner, w, case["truth"][b])
            # 4. the flung-out hypothesis: no pixel, never chosen, not counted
            assert rec[b].valid[hr.FLUNG] == 0 and rec[b].winner != hr.FLUNG and rec[b].num_eligible == len(scores) - 1 and rec[b].status == 0, b
            dt_ = float(np.abs(kt[b].ravel() - cands[b][w][0]).max())
            dR_ = float(np.abs(kR[b].ravel() - cands[b][w][1]).max())
            assert dt_ <= pt.algebra_bound("predict_knots_t") and dR_ <= pt.algebra_bound("predict_knots_R"), (b, dt_, dR_)
            if w == 0:
                assert kt[b].tobytes() == tkt[b].tobytes() and kR[b].tobytes() == tkR[b].tobytes(), b
            else:
                assert kt[b].tobytes() != tkt[b].tobytes(), b
        winners = [r.winner for r in rec]
        assert B == 1 or (0 in winners and any(w != 0 for w in winners)), winners
        # everything but the knots is what predict leaves
        assert _problem_times(pb) == _problem_times(twin)
        for a, t in zip(pb.get_states(), twin.get_states()):
            sa, st = pt.state_arrays(a), pt.state_arrays(t)
            assert all(np.array_equal(sa[key], st[key]) for key in ("velocity", "T_prev", "T_keyframe")) and sa["t0"] == st["t0"] \
                and sa["prev_timestamp"] == st["prev_timestamp"]
        # the LM that follows starts at the winner's cost
        res = (capi.LmBatchResult * B)()
        o = po.lm_opts(capi, k)
        assert gpu_ctx.lib.mbavo_lm_batch_levels(gpu_ctx.handle, B, L, pb.array, C.byref(o), res, None, 0) == 0
        torch.cuda.synchronize()
        for b in range(B):
            w = rec[b].winner
            KP = float(rec[b].num_keypoints) * hr.P
            want = rec[b].score[w] * rec[b].valid[w] / KP
            rel = abs(res[b].initial_cost - want) / abs(want)
            assert rel <= 1e-9, (b, res[b].initial_cost, want, rel)
            assert abs(res[b].initial_cost - oracle[b][3][w]) <= 1e-9 * abs(oracle[b][3][w]), b
        out = pb.commit(*THRESHOLDS)  # the call was a predict: the commit consumes it
        assert all(f.a.status == 0 for f in out)
    finally:
        pb.close()
        twin.close()


def test_min_gain_keeps_hypothesis_zero(orc, mbavo, gpu_ctx):
    B, H, W, k = hr.WIN_CASES[1]
    case = hr.win_case(orc, mbavo, B, H, W, k)
    states, cap, exp = case["states"], case["cap"], case["exp"]
    pb, twin = _prepared(gpu_ctx, case, states), _prepared(gpu_ctx, case, states)
    try:
        rec, oracle, _ = _check_scores(orc, mbavo, gpu_ctx, pb, states, cap, exp, hr.WIN_SCALES, hr.WIN_TWISTS, L - 1, "min_gain", min_gain=0.999)
        for b in range(B):  # (no challenger is a thousand times cheaper: by the oracle, with a margin far above the score bound)
            s = oracle[b][0]
            assert min(x for m, x in enumerate(s) if m >= 1 and oracle[b][2][m]) > 1.05 * 0.001 * s[0], b
        assert [r.winner for r in rec] == [0] * B and all(r.status == 0 for r in rec)
        assert twin.predict(cap, exp) == 0 and _snapshot(pb) == _snapshot(twin)
    finally:
        pb.close()
        twin.close()


# ---- 4. eligibility
def test_no_eligible_hypothesis_leaves_the_predict(orc, mbavo, gpu_ctx):
    """min_valid_frac = 1 on a pair that loses a pixel under every hypothesis (pair FAST, four times as fast), and a pair without a
    keypoint (pair BLANK, a blank keyframe): winner 0, MBAVO_HYP_NONE_ELIGIBLE, the knots of predict; the other pairs choose as the
    rule says (tests/pairs_hyp_ref.elig_case; the preconditions are asserted on the CPU)."""
    case, states = hr.elig_case(orc, mbavo)
    B, cap, exp = case["B"], case["cap"], case["exp"]
    scales, twists = hr.ELIG_SCALES, hr.ELIG_TWISTS
    pb, twin = _prepared(gpu_ctx, case, states), _prepared(gpu_ctx, case, states)
    try:
        assert pb.array[hr.BLANK * L + L - 1].K == 0 and pb.array[hr.FAST * L + L - 1].K > 0
        rec, oracle, _ = _check_scores(orc, mbavo, gpu_ctx, pb, states, cap, exp, scales, twists, L - 1, "eligibility", min_valid_frac=1.0)
        assert twin.predict(cap, exp) == 0
        for b in (hr.FAST, hr.BLANK):
            assert (rec[b].winner, rec[b].status, rec[b].num_eligible) == (0, hr.NONE_ELIGIBLE, 0), b
        assert rec[hr.BLANK].num_keypoints == 0 and rec[hr.FAST].valid[0] > 0
        kt, kR = pb.knots()
        tkt, tkR = twin.knots()
        for b in range(B):
            if rec[b].winner == 0:
                assert kt[b].tobytes() == tkt[b].tobytes() and kR[b].tobytes() == tkR[b].tobytes(), b
        others = [rec[b] for b in range(B) if b not in (hr.FAST, hr.BLANK)]
        assert all(r.status == 0 and r.num_eligible >= 1 for r in others) and any(r.winner != 0 for r in others)
        assert all(r.winner != hr.ELIG_FLUNG for r in rec)
    finally:
        pb.close()
        twin.close()


# ---- 6. repeatability and what the call costs
def test_same_bits_and_stats(orc, mbavo, gpu_ctx):
    capi = mbavo.capi
    B, H, W, k = hr.WIN_CASES[1]
    case, states = _assess_case(capi, B, H, W, k)
    scales, twists = _mixed(8, 5)
    pb = _prepared(gpu_ctx, case, states)
    try:
        plan_before = pb.stats()
        assert pb.hyp_stats() == (0, 0, 0)
        rc, rec = pb.predict_hypotheses(case["cap"], case["exp"], scales, twists, level=L - 1)
        assert rc == 0
        first = (bytes(rec), _snapshot(pb))
        launches = _launches_of_last_evaluation(gpu_ctx)
        assert pb.hyp_stats() == (2 + launches, 1, B * C.sizeof(capi.PairsHyp)), (pb.hyp_stats(), launches)
        assert pb.stats() == plan_before  # the scratch is not the plan's
        assert pb.set_states(states) == 0
        rc, none = pb.predict_hypotheses(case["cap"], case["exp"], scales, twists, level=L - 1, want_records=False)
        assert rc == 0 and none is None
        assert pb.hyp_stats() == (2 + launches, 0, 0)
        assert _snapshot(pb) == first[1]
        assert pb.set_states(states) == 0
        rc, again = pb.predict_hypotheses(case["cap"], case["exp"], scales, twists, level=L - 1)
        assert rc == 0 and (bytes(again), _snapshot(pb)) == first
        assert pb.track_stats() == ((0, 0, 0), (0, 0, 0))  # (predict's own witness is predict's)
    finally:
        pb.close()


# ---- 7. errors
def test_argument_errors_change_nothing(mbavo, gpu_ctx):
    capi, lib = mbavo.capi, gpu_ctx.lib
    B, H, W, k = 4, 120, 160, 2
    case, states = _assess_case(capi, B, H, W, k)
    cap, exp = np.ascontiguousarray(case["cap"]), np.ascontiguousarray(case["exp"])
    rec = (capi.PairsHyp * B)()
    pb = _batch(gpu_ctx, case)
    try:
        good = pb.hyp_opts([0.0, 2.0], [None, (0, 0, 0, 0, 0.01, 0)])

        def call(o=good, c=cap, e=exp, out=rec):
            return lib.mbavo_pairs_predict_hypotheses(pb.handle, capi.dp(np.ascontiguousarray(c)), capi.dp(np.ascontiguousarray(e)),
                                                      None if o is None else C.byref(o), out)

        def commit():
            return lib.mbavo_pairs_commit(pb.handle, ps.FLOW0, ps.FLOW1, ps.KERNEL, (capi.PairsFrame * B)())
        assert call() == E_ARG                                       # before the first prepare
        pb.prepare(*dv.dev(case["sharp"], case["depth"], case["blur"]))
        assert call() == E_ARG                                       # before the first set_states
        assert pb.set_states(states) == 0
        held = _snapshot(pb)

        def bad(**kw):
            o = pb.hyp_opts([0.0, 2.0], [None, (0, 0, 0, 0, 0.01, 0)])
            for key, v in kw.items():
                setattr(o, key, v)
            return o
        cases = [None, bad(M=0), bad(M=17), bad(M=-1), bad(level=-1), bad(level=L), bad(min_valid_frac=-0.1), bad(min_valid_frac=1.5),
                 bad(min_valid_frac=float("nan")), bad(min_gain=-0.1), bad(min_gain=1.0), bad(min_gain=float("nan")), bad(min_gain=float("inf"))]
        for v in (float("nan"), float("inf")):
            o = bad()
            o.scale[2] = v
            cases.append(o)
            o = bad()
            o.twist[1][4] = v
            cases.append(o)
        for i, o in enumerate(cases):
            assert call(o) == E_ARG, i
            assert _snapshot(pb) == held and commit() == E_ARG and pb.hyp_stats() == (0, 0, 0), i
        ok = bad()  # entries from M on and entry 0 are not read
        ok.scale[0], ok.scale[3], ok.twist[0][0], ok.twist[5][2] = float("nan"), float("inf"), float("nan"), float("nan")
        assert lib.mbavo_pairs_predict_hypotheses(pb.handle, None, capi.dp(exp), C.byref(good), rec) == E_ARG
        assert lib.mbavo_pairs_predict_hypotheses(pb.handle, capi.dp(cap), None, C.byref(good), rec) == E_ARG
        long_exp = exp.copy()
        long_exp[1] = (ps.N_KNOTS - 1) * case["dt"] + 0.2  # a blur sample outside the knots
        assert call(e=long_exp) == E_RANGE
        nan_cap = cap.copy()
        nan_cap[3] = np.nan
        assert call(c=nan_cap) == E_RANGE
        assert _snapshot(pb) == held and commit() == E_ARG and pb.hyp_stats() == (0, 0, 0)
        assert call(ok) == 0
        pending = _snapshot(pb)
        assert pending != held
        assert call() == E_ARG and pb.predict(cap, exp) == E_ARG     # a predict is pending
        assert _snapshot(pb) == pending
        assert commit() == 0 and commit() == E_ARG
    finally:
        pb.close()


# ---- 8. a camera set and the caller's points: the copied entries carry per-pair intrinsics and the caller's keypoints
def test_camera_set_object(orc, mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    B, H, W, k = hr.WIN_CASES[1]
    case, states = _assess_case(mbavo.capi, B, H, W, k)
    intr = case["intr"]
    to = [tuple(intr), (1.05 * intr[0], 0.95 * intr[1], intr[2] - 1.5, intr[3] + 1.0)]
    cam_of = [0, 1, 1, 0, 1, 0, 0]
    pb = _batch(gpu_ctx, case, num_cameras=2, undistort=0)
    try:
        cams = [workloads.pairs_camera(workloads.camera_radtan(H, W, intr, (0.0,) * 4), t) for t in to]
        assert pb.set_cameras(cams, cam_of) == 0
        pb.prepare(*dv.dev(case["sharp"], case["depth"], case["blur"]))
        assert pb.set_states(states) == 0
        for b in range(B):
            assert list(pb.array[b * L + 1].intrinsics) == [v / 2.0 for v in to[cam_of[b]]], b
        scales, twists = _mixed(4, 77)
        _check_scores(orc, mbavo, gpu_ctx, pb, states, case["cap"], case["exp"], scales, twists, 1, "camera set")
    finally:
        pb.close()


def test_points_object(orc, mbavo, gpu_ctx):
    B, H, W, k = hr.WIN_CASES[1]
    case, states = _assess_case(mbavo.capi, B, H, W, k)
    rng = np.random.default_rng(8)
    points = []
    for b in range(B):
        n = 90 + 10 * b
        xy = np.floor(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1))
        points.append((np.ascontiguousarray(xy), np.ascontiguousarray(rng.uniform(1.0, 3.0, n))))
    pb = _batch(gpu_ctx, case, every_candidate=True)
    try:
        sharp, _, blur = dv.dev(case["sharp"], case["depth"], case["blur"])
        counts = pb.prepare_points(sharp, blur, points)
        assert pb.set_states(states) == 0
        assert all(0 < counts[b, 1] <= len(points[b][1]) for b in range(B)) and len(set(counts[:, 1].tolist())) > 1
        scales, twists = _mixed(4, 78)
        _check_scores(orc, mbavo, gpu_ctx, pb, states, case["cap"], case["exp"], scales, twists, 1, "points")
    finally:
        pb.close()
