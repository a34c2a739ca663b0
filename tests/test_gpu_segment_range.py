"""Every API entry that relies on the spline's range gate (se3_math.h: spline_segment_checked, spline_segment_index), at the
times where a conversion to int decides nothing: NaN, +-inf, +-1e300, the times whose segment number is 2^31 - 4 (the index
plus k = 4 wraps) and 2^31, and 1.7e18 (nanosecond stamps on a spline in seconds); a good capture time with a NaN or infinite
exposure.  The gate itself is held to an exact reference, case by case, by tests/harness/segment_check.hip
(test_gpu_cxx_harness.py::test_segment_lookup_at_every_time, and tests/test_segment_host.py under the host sanitizers); here the
entries are held to what include/mbavo.h promises: MBAVO_E_RANGE, a context that is as good as new afterwards, and the one edge
that must not move -- a time up to one segment before the first knot is accepted, as the reference's truncation toward zero
accepts it, and exactly one segment before it is not.

mbavo_eval_batch is asynchronous: it returns before the device has seen the times, so it cannot return MBAVO_E_RANGE itself.
What the header promises for it is that the context's range status is raised and that the next call that synchronises reports
it once; that is what is asserted for it here (a good mbavo_eval behind it returns MBAVO_E_RANGE, the one after 0).

The scene is the one of test_gpu_fused.py::test_out_of_range_spline_is_reported (S = 8, F = 1, k = 4, P = 8, K = 50) with its k = 2
and S = 1 twins: t0 = 0, dt = 0.5, capture time 0.25, exposure 0.1.  The tests make their own contexts: an evaluation off the knots
raises the range status of its context, and the session's context is shared with tests that do not expect one.  The host-side
entries at the end need no GPU and are not marked."""
import ctypes as C

import numpy as np
import pytest

import eval_support as es
import lm_support as lms
import pairs_device as dv
import pairs_step as ps
import pairs_track as pt
import scenes
from mba_vo_amd import synth, workloads

gpu = pytest.mark.gpu
E_RANGE = -2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
T0, DT, CAP, EXP = 0.0, 0.5, 0.25, 0.1
NAN, INF = float("nan"), float("inf")
# capture times off the knots (name, value); the segment numbers 2^31 - 4 and 2^31 are exact: t0 = 0 and dt = 0.5
BAD_CAPS = [("nan", NAN), ("+inf", INF), ("-inf", -INF), ("1e300", 1e300), ("-1e300", -1e300), ("2^31-4", T0 + DT * (2.0 ** 31 - 4)),
            ("2^31", T0 + DT * 2.0 ** 31), ("1.7e18", 1.7e18)]
BAD_EXPS = [("exp nan", NAN), ("exp inf", INF)]
BAD_TIMES = [(name, v, EXP) for name, v in BAD_CAPS] + [(name, CAP, v) for name, v in BAD_EXPS]

# the engine options of tests/test_gpu_prologue_setup.py: pose entries by the fused kernel's prologue / by k_pose_table ahead of it
FORMS = {"default": {}, "prologue": dict(sample_parallel=-1, fused_pose=1, fused_pose_max_samples=21),
         "pose_kernel": dict(sample_parallel=-1, fused_pose=-1, fused_pose_max_samples=21)}
_SCENES = {}


def _scene(k, S, seed=0):
    """(Scene, DeviceScene), made once; the tests write cap and exp on the device and put them back."""
    key = (k, S, seed)
    if key not in _SCENES:
        sc = scenes.Scene(S=S, F=1, k=k, P=8, K=50, seed=seed)
        assert (sc.t0, sc.dt, float(sc.cap[0]), float(sc.exp[0]), sc.N) == (T0, DT, CAP, EXP, k)
        _SCENES[key] = (sc, scenes.DeviceScene(sc))
    return _SCENES[key]


def _set_times(d, cap, exp):
    import torch
    d.cap.copy_(torch.tensor([cap], dtype=torch.float64))
    d.exp.copy_(torch.tensor([exp], dtype=torch.float64))
    torch.cuda.synchronize()


def _eval(mbavo, ctx, sc, d, with_h):
    n = 6 * sc.N
    cost, H, g = np.zeros(1), (np.zeros(n * n) if with_h else None), (np.zeros(n) if with_h else None)
    p = d.problem()
    rc = ctx.lib.mbavo_eval(ctx.handle, C.byref(p), sc.k, mbavo.capi.dp(cost), mbavo.capi.dp(H), mbavo.capi.dp(g), None)
    return rc, cost, H, g


def _eval_batch(mbavo, ctx, k, ds, with_h):
    """mbavo_eval_batch and a synchronisation: (rc, the packed frame blocks as bytes)."""
    import torch
    B, E = len(ds), synth.packed_len(k)
    arr = (mbavo.capi.Problem * B)(*[d.problem() for d in ds])
    fb = torch.zeros(B * E, dtype=torch.float64, device="cuda:0")
    rc = ctx.lib.mbavo_eval_batch(ctx.handle, B, arr, k, 1 if with_h else 0, fb.data_ptr(), None, None)
    torch.cuda.synchronize()
    return rc, fb.cpu().numpy().tobytes()


@pytest.fixture()
def own_ctx(mbavo):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield ctx
    ctx.close()


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", [2, 4])
def test_evaluation_reports_every_time_off_the_knots(mbavo, own_ctx, k, form):
    """mbavo_eval returns MBAVO_E_RANGE for every bad time, with the pose entries made by the fused kernel's prologue, by k_pose_table
    and by whatever the default options choose, S = 1 and S = 8, H/g and cost-only; mbavo_eval_batch raises the range status.  The
    good calls afterwards give, through both entries, the bytes of a context with the same options that never saw a bad time."""
    import torch
    ctx = own_ctx
    fresh = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.engine_opts(**FORMS[form])
    fresh.engine_opts(**FORMS[form])
    for S in (1, 8):
        sc, d = _scene(k, S)
        try:
            for with_h in (True, False):
                assert _eval(mbavo, ctx, sc, d, with_h)[0] == 0
                kern = ctx.lib.mbavo_last_kernel(ctx.handle).decode()
                if form != "default":  # the witness of the form, as test_gpu_prologue_setup.py reads it
                    assert kern == "k_fused<%d,%s,false,%s>" % (k, "true" if with_h else "false", "true" if form == "prologue" else "false"), kern
                for name, cap, exp in BAD_TIMES:
                    _set_times(d, cap, exp)
                    assert _eval(mbavo, ctx, sc, d, with_h)[0] == E_RANGE, (name, S, with_h, kern)
                    assert _eval_batch(mbavo, ctx, k, [d], with_h)[0] == 0  # (asynchronous: the status is raised on the context ...)
                    _set_times(d, CAP, EXP)
                    assert _eval(mbavo, ctx, sc, d, with_h)[0] == E_RANGE, (name, S, with_h, kern, "the batch's status")  # ... reported once
                    assert _eval(mbavo, ctx, sc, d, with_h)[0] == 0, (name, S, with_h, kern)
                # the good calls afterwards: the bytes of a context that never saw a bad time, both entries
                got, want = _eval(mbavo, ctx, sc, d, with_h), _eval(mbavo, fresh, sc, d, with_h)
                assert got[0] == 0 and want[0] == 0 and got[1][0] > 0
                assert all(a is None and b is None or a.tobytes() == b.tobytes() for a, b in zip(got[1:], want[1:])), (S, with_h, kern)
                rc, got_b = _eval_batch(mbavo, ctx, k, [d], with_h)
                rc_f, want_b = _eval_batch(mbavo, fresh, k, [d], with_h)
                assert rc == 0 and rc_f == 0 and any(got_b) and got_b == want_b, (S, with_h, kern)
        finally:
            _set_times(d, CAP, EXP)
    fresh.close()


@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_a_bad_problem_in_the_middle_of_a_batch_and_the_context_afterwards(mbavo, own_ctx, k):
    """Three problems, the middle one's capture time bad: the range status is raised (the next synchronising call returns
    MBAVO_E_RANGE once).  Afterwards the good batch gives, on the same context, the bytes a fresh context gives."""
    import torch
    ctx = own_ctx
    fresh = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    trio = [_scene(k, 8, seed) for seed in (0, 1, 2)]
    ds = [d for _, d in trio]
    sc0, d0 = _scene(k, 1)
    try:
        for with_h in (True, False):
            for name, cap, exp in BAD_TIMES:
                _set_times(ds[1], cap, exp)
                assert _eval_batch(mbavo, ctx, k, ds, with_h)[0] == 0
                assert _eval(mbavo, ctx, sc0, d0, with_h)[0] == E_RANGE, (name, with_h)
                _set_times(ds[1], CAP, EXP)
                assert _eval(mbavo, ctx, sc0, d0, with_h)[0] == 0, (name, with_h)
                rc, got = _eval_batch(mbavo, ctx, k, ds, with_h)
                rc_f, want = _eval_batch(mbavo, fresh, k, ds, with_h)
                assert rc == 0 and rc_f == 0 and any(got) and got == want, (name, with_h)
    finally:
        _set_times(ds[1], CAP, EXP)
        fresh.close()


@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_one_segment_before_the_first_knot(orc, mbavo, own_ctx, k):
    """The edge that must not move.  Sample times in (t0 - dt, t0) truncate toward zero to segment 0 with u < 0: accepted, and the
    evaluation matches the oracle (which extrapolates the same way) within eval_support's tolerance.  A sample exactly at t0 - dt is
    off the knots.  S = 1: the one sample is at cap - exp / 2."""
    ctx = own_ctx
    sc = scenes.Scene(S=1, F=1, k=k, P=8, K=50, cap0=-0.2)  # sample time -0.25: tn = -0.5
    assert sc.N == k
    sc.start_idx[:] = 0
    d = scenes.DeviceScene(sc)
    got = scenes.gpu_eval(ctx, d)
    p, keep = sc.oracle_problem(orc)
    want = orc.evaluate(p)
    tol = es.tol(sc)
    assert es.rel(got["H"], want["H"]) <= tol and es.rel(got["g"], want["g"]) <= tol and abs(got["cost"] - want["cost"]) <= tol * abs(want["cost"])
    assert got["cost"] > 0
    for cap, rc_want in ((np.nextafter(-0.45, 0.0), 0), (-0.45, E_RANGE), (np.nextafter(0.05, -1.0), 0)):
        # tn = (cap - 0.05) / 0.5: just inside -1; -1 exactly (-0.45 - 0.05 rounds to -0.5); the last double below 0
        assert ((cap - 0.05) / 0.5 == -1.0) == (rc_want == E_RANGE)
        _set_times(d, cap, EXP)
        assert _eval(mbavo, ctx, sc, d, True)[0] == rc_want, cap


# ---- the batched LM
@gpu
@pytest.mark.parametrize("sync_every,groups", [(0, 1), (3, 2)])
def test_lm_batch_with_one_pair_off_the_knots(mbavo, sync_every, groups):
    """What test_gpu_lm_batch.py::test_lm_batch_failed_call_leaves_nothing_behind expects for its mild time, for every bad time: the
    call returns MBAVO_E_RANGE with nothing in flight, the good call afterwards repeats the first good call bit for bit, and an
    evaluation on the context gives the blocks of a fresh context."""
    import torch
    capi = mbavo.capi
    B, k, N, F = 3, 4, 4, 1
    probs = lms.scene(B, k, N, F, seed=83)
    o = lms.lm_batch_opts(capi, k, groups=groups, **dict(lms.OPTS, max_it=12))
    o.sync_every = sync_every
    stream = torch.cuda.current_stream().cuda_stream
    ctx, fresh = capi.Context(0, stream=stream), capi.Context(0, stream=stream)
    try:
        dw = workloads.DeviceWorkload(probs)
        rc_a, *rec_a, accepted = lms.lm_bits(capi, ctx, dw, probs, o)
        assert rc_a == 0 and accepted > 0
        good_cap, good_exp = dw.array[1].d_cap_time, dw.array[1].d_exp_time
        want = lms.eval_bits(fresh, dw, probs)
        for name, cap, exp in BAD_TIMES:
            bad = torch.tensor([cap if exp == EXP else exp], dtype=torch.float64, device="cuda:0")
            if exp == EXP:
                dw.array[1].d_cap_time = bad.data_ptr()
            else:
                dw.array[1].d_exp_time = bad.data_ptr()
            rc_bad = lms.lm_bits(capi, ctx, dw, probs, o)[0]
            assert rc_bad == E_RANGE, (name, rc_bad)
            assert torch.cuda.current_stream().query(), name               # nothing of the call is still in flight
            dw.array[1].d_cap_time, dw.array[1].d_exp_time = good_cap, good_exp
            rc_b, *rec_b, _ = lms.lm_bits(capi, ctx, dw, probs, o)
            assert rc_b == 0, (name, rc_b)
            assert rec_b[0] == rec_a[0] and rec_b[1] == rec_a[1] and rec_b[2] == rec_a[2], name
            blocks = lms.eval_bits(ctx, dw, probs)
            assert any(blocks) and blocks == want, name
        # the edge that must not move: every sample of pair 1 in (t0 - dt, t0) is accepted (segment 0, as its h_start_idx says);
        # the first sample exactly at t0 - dt is not.  S = 4, exposure 0.1: the samples span cap -+ 0.05
        for cap, rc_want in ((-0.2, 0), (-0.45, E_RANGE)):
            first = (cap - EXP * 0.5 - T0) / DT
            assert (first == -1.0) == (rc_want == E_RANGE) and -1.0 <= first and (cap + EXP * 0.5 - T0) / DT < 0.0
            edge = torch.tensor([cap], dtype=torch.float64, device="cuda:0")
            dw.array[1].d_cap_time = edge.data_ptr()
            assert lms.lm_bits(capi, ctx, dw, probs, o)[0] == rc_want, cap
            dw.array[1].d_cap_time = good_cap
        rc_b, *rec_b, _ = lms.lm_bits(capi, ctx, dw, probs, o)
        assert rc_b == 0 and rec_b[0] == rec_a[0] and rec_b[1] == rec_a[1] and rec_b[2] == rec_a[2]
    finally:
        ctx.close()
        fresh.close()


# ---- the pairs batch
PB, PL, PH, PW, PS_ = 2, 1, 120, 160, 4


def _pairs_inputs():
    rng = np.random.default_rng(24)
    sharp = np.stack([synth.texture_image(PH, PW, seed=40 + 3 * b, octaves=(32, 16, 8, 4)) for b in range(PB)])
    blur = np.stack([np.clip(np.roll(sharp[b], (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, (PH, PW)), 0, 255).astype(np.uint8) for b in range(PB)])
    depth = rng.uniform(1.0, 3.0, (PB, PH, PW)).astype(np.float32)
    return np.ascontiguousarray(sharp), depth, np.ascontiguousarray(blur)


def _pairs_motion(N):
    kt, kR = np.zeros((PB, N, 3)), np.zeros((PB, N, 4))
    for b in range(PB):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
    return dict(cap=np.array([0.1875, 0.25]), exp=np.full(PB, 0.0625), t0=np.zeros(PB), dt=DT, kt=kt, kR=kR)  # (binary fractions: the edges below are exact)


def _report(ctx, pb):
    import torch
    nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
    assert ctx.lib.mbavo_pairs_plan(C.byref(pb.opts), C.byref(nbytes), cells) == 0
    pc = torch.full((pb.B, cells[0]), -7.0, dtype=torch.float64, device="cuda:0")
    fl = torch.full((pb.B, cells[0]), 9, dtype=torch.uint8, device="cuda:0")
    out = pb.report(3.0, pc, fl)
    return out, pc.cpu().numpy(), fl.cpu().numpy()


@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_pairs_report_and_set_motion_off_the_knots(mbavo, own_ctx, k):
    """Pair 1's times are moved off its knots through mbavo_pairs_set_states (its start time: the capture time minus the bad
    segment number times dt, or the bad value itself): the report says MBAVO_E_RANGE with the NaN-filled record that
    test_gpu_pairs_report.py::test_a_capture_time_off_the_knots_and_a_pair_at_rest asserts, pair 0 as without it.
    mbavo_pairs_set_motion refuses the same times itself with MBAVO_E_RANGE, the previous motion left in place."""
    capi, ctx, N = mbavo.capi, own_ctx, k
    m = _pairs_motion(N)
    pb = workloads.PairBatch(ctx, PB, L=PL, H=PH, W=PW, S=PS_, k=k, N=N, cell=12, thresh=4.0, border=4)
    try:
        counts = pb.prepare(*dv.dev(*_pairs_inputs()))
        assert counts[1, 0] > 0
        assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        case = dict(B=PB, kt=m["kt"], kR=m["kR"], t0=m["t0"], dt=m["dt"], cap=m["cap"])
        assert pb.set_states(pt.make_states(capi, case)) == 0
        good, gpc, gfl = _report(ctx, pb)
        assert [good[b].status for b in range(PB)] == [0, 0]
        cap1 = float(m["cap"][1])
        # start times that put pair 1's capture time at the bad segment numbers: NaN, +-inf, +-1e300 / dt, 2^31 - 4, 2^31, 1.7e18 / dt
        starts = [("nan", NAN), ("+inf", -INF), ("-inf", INF), ("1e300", -1e300), ("-1e300", 1e300), ("2^31-4", cap1 - DT * (2.0 ** 31 - 4)),
                  ("2^31", cap1 - DT * 2.0 ** 31), ("1.7e18", -1.7e18)]
        for name, t0 in starts:
            tn = (cap1 - t0) / DT
            assert not (-1.0 < tn < 2.0 ** 31 - 8), (name, tn)  # (what this test builds: NaN, or a segment number far off N = k)
            assert pb.set_states(pt.make_states(capi, dict(case, t0=np.array([0.0, t0])))) == 0
            out, pc, fl = _report(ctx, pb)
            r = out[1]
            assert r.status == E_RANGE and r.num_keypoints0 == counts[1, 0] and r.num_flagged == 0 and r.num_stat == 0, (name, r.status)
            doubles = np.frombuffer(bytes(r), np.float64)[2:]
            assert np.isnan(doubles).all() and (pc[1] == -7.0).all() and (fl[1] == 9).all(), name
            assert bytes(out[0]) == bytes(good[0]) and np.array_equal(pc[0], gpc[0]) and np.array_equal(fl[0], gfl[0]), name
        # the edge that must not move: pair 1's capture time and samples in (t0 - dt, t0) are accepted, the capture time exactly at
        # t0 - dt is not (cap 0.25, samples 0.25 -+ 0.03125, dt 0.5)
        for t0, status_want in ((0.5, 0), (0.75, E_RANGE)):
            assert ((cap1 - t0) / DT == -1.0) == (status_want == E_RANGE) and (status_want != 0 or -1.0 < (cap1 - 0.03125 - t0) / DT) and (cap1 + 0.03125 - t0) / DT < 0.0
            assert pb.set_states(pt.make_states(capi, dict(case, t0=np.array([0.0, t0])))) == 0
            out, pc, fl = _report(ctx, pb)
            assert (out[1].status == E_RANGE) == (status_want == E_RANGE), (t0, out[1].status)
            if status_want == 0:
                assert np.isfinite(np.array(out[1].T)).all() and out[1].cost > 0 and (pc[1, :counts[1, 0]] >= 0).all()
            assert bytes(out[0]) == bytes(good[0]), t0
        # set_motion: the host's check of the same sample times, nothing touched
        assert pb.set_states(pt.make_states(capi, case)) == 0
        for name, cap, exp in BAD_TIMES:
            caps, exps = m["cap"].copy(), m["exp"].copy()
            caps[1], exps[1] = (cap, exps[1]) if exp == EXP else (caps[1], exp)
            assert pb.set_motion(caps, exps, m["t0"], m["dt"], 2.0 * m["kt"], m["kR"]) == E_RANGE, name
        # (its first sample exactly at t0 - dt: cap - exp / 2 = -0.5)
        caps = m["cap"].copy()
        caps[1] = -0.46875
        assert (caps[1] - 0.0625 * 0.5) / DT == -1.0
        assert pb.set_motion(caps, m["exp"], m["t0"], m["dt"], 2.0 * m["kt"], m["kR"]) == E_RANGE
        out, pc, fl = _report(ctx, pb)
        assert all(bytes(out[b]) == bytes(good[b]) for b in range(PB)) and np.array_equal(pc, gpc) and np.array_equal(fl, gfl)
        # ... and accepts samples in (t0 - dt, t0): the motion is taken (the report changes)
        caps[1] = -0.25
        assert pb.set_motion(caps, m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        out, pc, fl = _report(ctx, pb)
        assert out[1].status != E_RANGE and np.isfinite(np.array(out[1].T)).all() and bytes(out[1]) != bytes(good[1]) and bytes(out[0]) == bytes(good[0])
    finally:
        pb.close()


# ---- the host-driven LM loop: the times are checked on the host before anything is launched
@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_optimize_trajectory_off_the_knots(mbavo, own_ctx, k):
    capi, ctx = mbavo.capi, own_ctx
    p = lms.scene(1, k, 4, 1, seed=91)[0]
    dw = workloads.DeviceWorkload([p])
    lv = (capi.Level * 1)()
    q, a = lv[0], dw.array[0]
    q.H, q.W, q.K, q.P, q.S = p.H, p.W, p.K, p.P, p.S
    q.d_ref_img, q.d_ref_dIxy, q.d_cur_imgs = a.d_ref_img, a.d_ref_dIxy, a.d_cur_imgs
    q.d_kp_xy, q.d_kp_z, q.d_pattern = a.d_kp_xy, a.d_kp_z, a.d_pattern
    o = capi.TrackOpts()
    o.num_levels, o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = 1, k, 3, 5
    for i in range(4):
        o.intrinsics[i] = float(p.intr[i])
    o.huber_k, o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = p.huber, 0.5, 1e-3, 3.0

    def call(cap, exp):
        kt, kR, caps, exps = p.knots_t.copy(), p.knots_R.copy(), np.array([cap]), np.array([exp])
        start, cost, trace = np.zeros(1, np.int32), np.zeros(1), (capi.TraceRec * 16)()
        rc = ctx.lib.mbavo_optimize_trajectory(ctx.handle, C.byref(o), lv, 1, capi.dp(caps), capi.dp(exps), p.t0, p.dt,
                                               capi.dp(kt), capi.dp(kR), p.N, capi.ip(start), capi.dp(cost), trace, 16)
        return rc, kt, kR

    assert (p.t0, p.dt) == (T0, DT)
    assert call(float(p.cap[0]), float(p.exp[0]))[0] > 0
    for name, cap, exp in BAD_TIMES:
        rc, kt, kR = call(cap, exp)
        assert rc == E_RANGE and np.array_equal(kt, p.knots_t) and np.array_equal(kR, p.knots_R), (name, rc)
    assert call(float(p.cap[0]), float(p.exp[0]))[0] > 0
    # the edge that must not move (S = 4, exposure 0.1): samples in (t0 - dt, t0) run, the first sample exactly at t0 - dt does not
    assert float(p.exp[0]) == EXP and (-0.45 - EXP * 0.5) / DT == -1.0 and (np.nextafter(-0.45, 0.0) - EXP * 0.5) / DT > -1.0
    rc, kt, kR = call(-0.2, EXP)
    assert rc > 0 and np.isfinite(kt).all() and np.isfinite(kR).all(), rc
    assert call(float(np.nextafter(-0.45, 0.0)), EXP)[0] > 0
    assert call(-0.45, EXP)[0] == E_RANGE


# ---- the reference's launcher: no knot count in its signature
@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_compute_virtual_camera_poses_at_every_time(mbavo, own_ctx, k):
    """mbavo_compute_virtual_camera_poses (k_api_poses) has no range to report and no knot count to clamp against.  A NaN or infinite
    time (from the capture or the exposure time) and a time whose segment number fits no int give NaN in every output, no knot read;
    a time with a negative segment number is evaluated at the start of segment 0; in range, (t0 - dt, t0) included, the pose is
    mbavo_spline_get_pose's.  S = 1 and exposure 0: the sample time is the capture time."""
    import torch
    capi, N = mbavo.capi, k + 3
    kt, kR = synth.harness_spline(0.004, 0.05, N)
    kt, kR = np.ascontiguousarray(kt.ravel()), np.ascontiguousarray(kR.ravel())
    # (no time between the knots' end and segment number 2^31 - k: the launcher cannot know where the knots end and reads there)
    nan_caps = [NAN, INF, -INF, 1e300, -1e300, 1.7e18, -1.7e18, DT * 2.0 ** 31, -DT * (2.0 ** 31 + 1), CAP, CAP]
    nan_exps = [0.0] * (len(nan_caps) - 2) + [NAN, INF]
    start_caps = [-0.5, -1.6, -DT * 2.0 ** 31]   # segment numbers -1, -3 (and a fraction), INT_MIN: the start of segment 0
    good_caps = [-0.25, float(np.nextafter(-0.5, 0.0)), -5e-324, 0.0, 0.3, 1.1, float(np.nextafter(DT * (N - k + 1), 0.0))]
    caps = np.array(nan_caps + start_caps + good_caps)
    exps = np.array(nan_exps + [0.0] * (len(start_caps) + len(good_caps)))
    F = caps.size
    d_cap, d_exp, d_kt, d_kR = dv.dev(caps, exps, kt, kR)
    poses = torch.full((F, 7), 5.0, dtype=torch.float64, device="cuda:0")
    Jt = torch.full((F, 9 * k), 5.0, dtype=torch.float64, device="cuda:0")
    JR = torch.full((F, 12 * k), 5.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for with_j in (True, False):
        assert own_ctx.lib.mbavo_compute_virtual_camera_poses(1, F, d_cap.data_ptr(), d_exp.data_ptr(), k, T0, DT, d_kt.data_ptr(), d_kR.data_ptr(),
                                                              poses.data_ptr(), Jt.data_ptr() if with_j else None, JR.data_ptr() if with_j else None) == 0
        got, gJt, gJR = poses.cpu().numpy(), Jt.cpu().numpy(), JR.cpu().numpy()
        n = len(nan_caps)
        assert np.isnan(got[:n]).all() and np.isnan(gJt[:n]).all() and np.isnan(gJR[:n]).all()
        assert np.isfinite(got[n:]).all() and np.isfinite(gJt[n:]).all() and np.isfinite(gJR[n:]).all()
        for i in range(n, F):
            t = T0 if i < n + len(start_caps) else float(caps[i])
            p, q, jt, jr = np.zeros(3), np.zeros(4), np.zeros(9 * k), np.zeros(12 * k)
            assert own_ctx.lib.mbavo_spline_get_pose(k, T0, DT, capi.dp(kt), capi.dp(kR), N, t, capi.dp(p), capi.dp(q), capi.dp(jt), capi.dp(jr)) == 0, t
            assert np.abs(got[i] - np.r_[p, q]).max() <= 1e-12, (caps[i], got[i], p, q)
            assert np.abs(gJt[i] - jt).max() <= 1e-12 and np.abs(gJR[i] - jr).max() <= 1e-12, caps[i]


# ---- host entries: no launch, no GPU
def _get_pose(mbavo, k, N, t, t0=T0, dt=DT):
    kt, kR = synth.harness_spline(0.004, 0.05, N)
    kt, kR = np.ascontiguousarray(kt.ravel()), np.ascontiguousarray(kR.ravel())
    p, q = np.full(3, 7.0), np.full(4, 7.0)
    rc = mbavo.load().mbavo_spline_get_pose(k, t0, dt, mbavo.capi.dp(kt), mbavo.capi.dp(kR), N, float(t), mbavo.capi.dp(p), mbavo.capi.dp(q), None, None)
    return rc, p, q


@pytest.mark.parametrize("k", [2, 4])
def test_spline_get_pose_off_the_knots(mbavo, k):
    """SplineSE3::GetPose behind mbavo_spline_get_pose: MBAVO_E_RANGE for every bad time, outputs untouched; a time in (t0 - dt, t0)
    is accepted, t0 - dt exactly is not; the last segment ends where the knots end."""
    for N in (k, k + 3):
        for name, t in BAD_CAPS:
            rc, p, q = _get_pose(mbavo, k, N, t)
            assert rc == E_RANGE and (p == 7.0).all() and (q == 7.0).all(), (name, N)
        for t, want in ((-0.25, 0), (np.nextafter(-0.5, 0.0), 0), (-0.5, E_RANGE), (0.0, 0), (-0.0, 0), (5e-324, 0), (-5e-324, 0),
                        (np.nextafter(DT * (N - k + 1), 0.0), 0), (DT * (N - k + 1), E_RANGE)):
            rc, p, q = _get_pose(mbavo, k, N, t)
            assert rc == want, (t, N, rc)
            if want == 0:
                assert np.isfinite(p).all() and abs(np.linalg.norm(q) - 1.0) < 1e-12, (t, N)


def test_segment_start_index_for_every_double(mbavo):
    """mbavo_segment_start_index: trunc((t - t0) / dt) held to [INT_MIN, INT_MAX], INT_MIN for NaN."""
    f = mbavo.load().mbavo_segment_start_index
    cases = [(NAN, INT_MIN), (INF, INT_MAX), (-INF, INT_MIN), (1e300, INT_MAX), (-1e300, INT_MIN), (1.7e18, INT_MAX), (-1.7e18, INT_MIN),
             (DT * (2.0 ** 31 - 4), 2 ** 31 - 4), (DT * (2.0 ** 31 - 1), INT_MAX), (DT * (2.0 ** 31 - 0.5), INT_MAX), (DT * 2.0 ** 31, INT_MAX),
             (DT * (2.0 ** 31 + 1), INT_MAX), (DT * -(2.0 ** 31), INT_MIN), (DT * -(2.0 ** 31 + 0.5), INT_MIN), (DT * -(2.0 ** 31 + 1), INT_MIN),
             (DT * -(2.0 ** 31 - 1), INT_MIN + 1), (0.0, 0), (-0.0, 0), (-0.15, 0), (-0.5, -1), (-0.75, -1), (0.25, 0), (1.85, 3), (1.5, 3)]
    for t, want in cases:
        assert f(float(t), T0, DT) == want, (t, want)
    assert f(0.25, NAN, DT) == INT_MIN and f(0.25, T0, NAN) == INT_MIN and f(0.25, T0, 0.0) == INT_MAX and f(-0.25, T0, 0.0) == INT_MIN
    assert f(0.0, T0, 0.0) == INT_MIN  # 0 / 0
    # with a start time and a spacing that are not binary fractions: the truncation of the double quotient
    for t in (1.7e9 + 0.3, 1.7e9 + 33.0 / 30.0, 1.7e9 - 0.01):
        assert f(t, 1.7e9, 1.0 / 30.0) == int((t - 1.7e9) / (1.0 / 30.0))
