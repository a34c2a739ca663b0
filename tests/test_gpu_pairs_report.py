"""mbavo_pairs_report on the device, through the C ABI, against the numpy restatement (tests/pairs_report_ref.py, itself held to the
library's spline code and to the oracle by tests/test_pairs_report_api.py) fed with a separate mbavo_eval_batch of the same level-0
problems.

Shapes: B = 3 pairs of 120 x 160 textures at L = 2, S = 4, the 8-pixel pattern, grid cells of 12 (level-0 K around 100, no multiple
of 64); an every-candidate object (K > 4096: more than sixteen strides of the workgroup); K = 0 (an all-zero depth map).

Bounds.  info_unit: elementwise gamma_n (|A|^T |H| |A|) K P with n = 2 6k + 2 (pairs_report_ref.info_bound) -- A is formed with the
same operations on both sides.  sigma2: three roundings, 4 2^-53 relative.  cost, num_valid_px and the patch costs: the
evaluation's bits.  T: the bits of mbavo_pairs_assess (the same device function).  cov: against the inverse formed in numpy
longdouble; the yardstick is the error of the restatement's own float64 Cholesky inverse against that, the device gets 8 times the
yardstick (its sums run with the same algorithm in another order, with contraction off) and never less than 64 2^-53 relative to
the largest entry (a yardstick that happens to round well is not a bound).  Measured: profiles/r24_pairs_report.txt."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_device as dv
import pairs_report_ref as rr
import pairs_step as ps
import pairs_track as pt
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, SINGULAR = -1, -2, 1
B, L, H, W, S, P, CELL, THR = 3, 2, 120, 160, 4, 8, 12, 4.0
U = 2.0 ** -53
_CASE = {}


def _case():
    """Three pairs: the blurred frame is the keyframe shifted by a pixel with a little noise; pair 1's has a pasted occluder."""
    if not _CASE:
        rng = np.random.default_rng(24)
        sharp = np.stack([synth.texture_image(H, W, seed=40 + 3 * b, octaves=(32, 16, 8, 4)) for b in range(B)])
        blur = np.stack([np.clip(np.roll(sharp[b], (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8) for b in range(B)])
        blur[1, 30:70, 50:100] = synth.texture_image(40, 50, seed=99, octaves=(8, 4))
        depth = rng.uniform(1.0, 3.0, (B, H, W)).astype(np.float32)
        _CASE.update(sharp=np.ascontiguousarray(sharp), blur=np.ascontiguousarray(blur), depth=depth)
    return _CASE


def _motion(k, N, start, seed=0):
    """Times and knots with every blur sample and the capture time on segment `start`."""
    rng = np.random.default_rng(7 + seed)
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.05, 3)  # (a translation of some size: the -[t]x columns of A carry weight)
    cap = (start + 0.4 + 0.05 * np.arange(B)) * 0.5
    return dict(cap=cap, exp=np.full(B, 0.04), t0=np.zeros(B), dt=0.5, kt=kt, kR=kR)


def _object(ctx, k, N, pairs=B, dense=False, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, pairs, L=L, H=H, W=W, S=S, k=k, N=N, cell=0 if dense else CELL, thresh=THR, border=4, every_candidate=dense, **kw)


def _cap0(ctx, pb):
    nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
    assert ctx.lib.mbavo_pairs_plan(C.byref(pb.opts), C.byref(nbytes), cells) == 0
    return cells[0], nbytes.value


def _prepared(ctx, k, N, start, sel=slice(None), dense=False, depth=None, blur=None):
    c, m = _case(), _motion(k, N, start)
    n = len(range(B)[sel])
    pb = _object(ctx, k, N, pairs=n, dense=dense)
    d = c["depth"] if depth is None else depth
    bl = c["blur"] if blur is None else blur
    counts = pb.prepare(*dv.dev(np.ascontiguousarray(c["sharp"][sel]), np.ascontiguousarray(d[sel]), np.ascontiguousarray(bl[sel])))
    assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    return pb, counts, {key: (v[sel] if isinstance(v, np.ndarray) else v) for key, v in m.items()}


def _launches_of_last_evaluation(ctx):
    """The header's rule on the engine's witnesses."""
    name = ctx.lib.mbavo_last_kernel(ctx.handle).decode()
    lay = (C.c_int * 8)()
    assert ctx.lib.mbavo_last_layout(ctx.handle, lay) == 0
    if name.startswith("k_fused_sp<") and name.endswith(",true>"):
        return 1
    return (0 if name.endswith(",true>") else 1) + (1 if lay[0] > 0 else 0) + 1


def _separate_eval(mbavo, ctx, pb, k):
    """mbavo_eval_batch(with_hessian = 1) on copies of the level-0 entries: (blocks n x E, patch costs per pair, valid n, launches)."""
    import torch
    capi, n = mbavo.capi, pb.B
    arr = (capi.Problem * n)()
    for b in range(n):
        C.memmove(C.byref(arr[b]), C.byref(pb.array[b * pb.L]), C.sizeof(capi.Problem))
        assert not arr[b].d_outlier and arr[b].num_bad == 0 and arr[b].num_residuals == 0
    Ks = [arr[b].K for b in range(n)]
    E = rr.packed_len(k)
    fb = torch.zeros(n * E, dtype=torch.float64, device="cuda:0")
    pc = torch.zeros(max(sum(Ks), 1), dtype=torch.float64, device="cuda:0")
    valid = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    capi.check(ctx.lib.mbavo_eval_batch(ctx.handle, n, arr, k, 1, fb.data_ptr(), pc.data_ptr(), valid.data_ptr()), "mbavo_eval_batch")
    torch.cuda.synchronize()
    launches = _launches_of_last_evaluation(ctx)
    off = np.concatenate([[0], np.cumsum(Ks)])
    pcs = pc.cpu().numpy()
    return fb.cpu().numpy().reshape(n, E), [pcs[off[b]:off[b + 1]] for b in range(n)], valid.cpu().numpy(), launches


def _report(ctx, pb, chi=3.0, fill=-7.0):
    import torch
    cap0 = _cap0(ctx, pb)[0]
    pc = torch.full((pb.B, cap0), fill, dtype=torch.float64, device="cuda:0")
    fl = torch.full((pb.B, cap0), 9, dtype=torch.uint8, device="cuda:0")
    out = pb.report(chi, pc, fl)
    return out, pc.cpu().numpy(), fl.cpu().numpy()


def _check_against_restatement(mbavo, ctx, pb, counts, m, k, start, tag, after_lm=False):
    out, pc, fl = _report(ctx, pb)
    blocks, costs, valid, _ = _separate_eval(mbavo, ctx, pb, k)
    assess = pb.assess(ps.FLOW0, ps.FLOW1, ps.KERNEL)
    worst = dict(info=0.0, sigma2=0.0, cov=0.0, cov_yard=0.0)
    for b in range(pb.B):
        r, K = out[b], int(counts[b, 0])
        want = rr.report(blocks[b], m["kt"][b][start:start + k], m["kR"][b][start:start + k], costs[b], valid[b], K, P, k, 3.0)
        assert r.num_keypoints0 == K and K % 64 != 0 and K > 64, (tag, b, K)
        if after_lm and (r.status != 0 or want["status"] != 0):
            # an alignment of these synthetic pairs may end far from the truth, with an information matrix that is singular to
            # working precision: whether a pivot comes out <= 0 is then decided by rounding, and only that is accepted here
            assert np.linalg.cond(want["info_unit"]) > 1e12 and r.status in (0, SINGULAR), (tag, b, r.status)
            continue
        assert r.status == want["status"] == 0, (tag, b, r.status)
        assert r.cost == want["cost"] == blocks[b][0] and r.num_valid_px == valid[b] and valid[b] > 6, (tag, b)  # bit for bit
        assert np.array_equal(pc[b, :K], costs[b]) and (pc[b, K:] == -7.0).all(), (tag, b)
        assert bytes(r.T) == bytes(assess[b].T) and assess[b].status == 0, (tag, b)
        p, q = np.zeros(3), np.zeros(4)
        assert ctx.lib.mbavo_spline_get_pose(k, 0.0, m["dt"], mbavo.capi.dp(np.ascontiguousarray(m["kt"][b])), mbavo.capi.dp(np.ascontiguousarray(m["kR"][b])),
                                             m["kt"].shape[1], float(m["cap"][b]), mbavo.capi.dp(p), mbavo.capi.dp(q), None, None) == 0
        assert np.abs(np.array(r.T) - np.r_[p, q]).max() <= 1e-12, (tag, b)
        info = np.array(r.info_unit).reshape(6, 6)
        bound = rr.info_bound(want["H"], want["A"], K, P)
        ratio = float((np.abs(info - want["info_unit"]) / bound).max())
        worst["info"] = max(worst["info"], ratio)
        assert ratio <= 1.0 and np.array_equal(info, info.T), (tag, b, ratio)
        rel = abs(r.sigma2 - want["sigma2"]) / want["sigma2"]
        worst["sigma2"] = max(worst["sigma2"], rel)
        assert rel <= 4 * U, (tag, b, rel)
        # cov: the device's inverse of ITS info_unit against longdouble
        ld = rr.cov(info, r.sigma2, np.longdouble)
        yard = float(np.abs(rr.cov(info, r.sigma2) - ld).max() / np.abs(ld).max())
        cov = np.array(r.cov).reshape(6, 6)
        err = float(np.abs(cov - ld).max() / np.abs(ld).max())
        worst["cov"], worst["cov_yard"] = max(worst["cov"], err), max(worst["cov_yard"], yard)
        assert err <= max(8 * yard, 64 * U) and np.array_equal(cov, cov.T), (tag, b, err, yard)
        # flags: the restatement on the device's own costs
        near = rr.near_the_bound(pc[b, :K], want["mu"], want["bound"], K)
        assert not near.any(), (tag, b)
        assert np.array_equal(fl[b, :K], want["flags"]) and (fl[b, K:] == 9).all(), (tag, b)
        assert (r.num_flagged, r.num_stat) == (want["num_flagged"], want["num_stat"]), (tag, b)
    print("report %s: info_unit error / bound %.3f, sigma2 rel %.2e, cov rel %.3e (float64 yardstick %.3e), flagged %s"
          % (tag, worst["info"], worst["sigma2"], worst["cov"], worst["cov_yard"], [out[b].num_flagged for b in range(pb.B)]))
    return out


# ---- checks 1, 2, 3 and 4
@pytest.mark.parametrize("k,extra,start", [(2, 0, 0), (4, 0, 0), (2, 2, 1), (4, 2, 1)])
def test_the_record_against_the_restatement(mbavo, gpu_ctx, k, extra, start):
    pb, counts, m = _prepared(gpu_ctx, k, k + extra, start)
    try:
        out = _check_against_restatement(mbavo, gpu_ctx, pb, counts, m, k, start, "k=%d N=%d start=%d" % (k, k + extra, start))
        assert out[1].num_flagged > 0 and out[1].num_flagged < counts[1, 0]  # the occluder
        # after an alignment the knots have moved: the same agreement at the LM's knots
        res = (mbavo.capi.LmBatchResult * B)()
        o = lms.lm_batch_opts(mbavo.capi, k, 3)
        assert gpu_ctx.lib.mbavo_lm_batch_levels(gpu_ctx.handle, B, L, pb.array, C.byref(o), res, None, 0) == 0
        kt, kR = pb.knots()
        assert not np.array_equal(kt, m["kt"])
        _check_against_restatement(mbavo, gpu_ctx, pb, counts, dict(m, kt=kt, kR=kR), k, start, "k=%d N=%d after the LM" % (k, k + extra), after_lm=True)
    finally:
        pb.close()


# ---- check 5
def test_every_candidate_and_a_pair_without_keypoints(mbavo, gpu_ctx):
    c = _case()
    depth = c["depth"].copy()
    depth[2] = 0.0
    pb, counts, m = _prepared(gpu_ctx, 2, 2, 0, dense=True, depth=depth)
    try:
        assert counts[0, 0] > 4096 and counts[1, 0] > 4096 and counts[2, 0] == 0 and counts[0, 0] % 256 != 0
        out, pc, fl = _report(gpu_ctx, pb)
        blocks, costs, valid, _ = _separate_eval(mbavo, gpu_ctx, pb, 2)
        for b in range(2):
            K = int(counts[b, 0])
            want = rr.report(blocks[b], m["kt"][b], m["kR"][b], costs[b], valid[b], K, P, 2, 3.0)
            assert out[b].status == 0 and out[b].cost == want["cost"] and np.array_equal(pc[b, :K], costs[b]) and (pc[b, K:] == -7.0).all()
            near = rr.near_the_bound(costs[b], want["mu"], want["bound"], K)
            assert not near.any() and np.array_equal(fl[b, :K], want["flags"]) and (fl[b, K:] == 9).all()
            assert (out[b].num_flagged, out[b].num_stat) == (want["num_flagged"], want["num_stat"]) and out[b].num_flagged > 0
            info = np.array(out[b].info_unit).reshape(6, 6)
            assert (np.abs(info - want["info_unit"]) <= rr.info_bound(want["H"], want["A"], K, P)).all()
        r = out[2]
        assert r.status == SINGULAR and r.num_keypoints0 == 0 and r.num_flagged == 0 and r.num_stat == 0 and r.cost == 0.0 and r.num_valid_px == 0.0
        assert np.isnan(np.array(r.cov)).all() and (np.array(r.info_unit) == 0.0).all() and r.sigma2 == 0.0
        assert (pc[2] == -7.0).all() and (fl[2] == 9).all()
    finally:
        pb.close()


def test_a_capture_time_off_the_knots_and_a_pair_at_rest(mbavo, gpu_ctx):
    """Pair 1's start time is moved behind its capture time through mbavo_pairs_set_states (set_motion and predict refuse such
    times themselves): MBAVO_E_RANGE and NaN, the neighbours as without it.  Pair 2's blurred frame is its keyframe at identity
    motion: every patch cost is below 1e-8, num_stat = 0, nothing flagged."""
    capi, c, k, N = mbavo.capi, _case(), 2, 2
    blur = c["blur"].copy()
    blur[2] = c["sharp"][2]
    pb, counts, m = _prepared(gpu_ctx, k, N, 0, blur=blur)
    try:
        m["kt"][2], m["kR"][2] = 0.0, np.array([0.0, 0.0, 0.0, 1.0])
        assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        good, gpc, gfl = _report(gpu_ctx, pb)
        assert [good[b].status for b in range(B)] == [0, 0, 0] or good[2].status == SINGULAR
        assert good[2].num_stat == 0 and good[2].num_flagged == 0 and (gfl[2, :counts[2, 0]] == 0).all()
        # (not exactly 0: the samples' interpolation weights round; every cost is far below the statistic's 1e-8)
        assert (gpc[2, :counts[2, 0]] < 1e-8).all() and (gpc[2, :counts[2, 0]] >= 0.0).all() and counts[2, 0] > 0 and good[2].cost < 1e-8
        case = dict(B=B, kt=m["kt"], kR=m["kR"], t0=np.array([0.0, 5.0, 0.0]), dt=m["dt"], cap=m["cap"])
        assert pb.set_states(pt.make_states(capi, case)) == 0
        out, pc, fl = _report(gpu_ctx, pb)
        r = out[1]
        assert r.status == E_RANGE and r.num_keypoints0 == counts[1, 0] and r.num_flagged == 0 and r.num_stat == 0
        doubles = np.frombuffer(bytes(r), np.float64)[2:]
        assert np.isnan(doubles).all() and (pc[1] == -7.0).all() and (fl[1] == 9).all()
        for b in (0, 2):
            assert bytes(out[b]) == bytes(good[b]) and np.array_equal(pc[b], gpc[b]) and np.array_equal(fl[b], gfl[b]), b
        # the evaluation clamped pair 1's samples and raised the context's range status, as any evaluation off the knots does: the
        # next LM call on the context reports it once (the header says so), the one after runs
        assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        o, res = lms.lm_batch_opts(capi, k, 3), (capi.LmBatchResult * B)()
        assert gpu_ctx.lib.mbavo_lm_batch_levels(gpu_ctx.handle, B, L, pb.array, C.byref(o), res, None, 0) == E_RANGE
        assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
        assert gpu_ctx.lib.mbavo_lm_batch_levels(gpu_ctx.handle, B, L, pb.array, C.byref(o), res, None, 0) == 0
    finally:
        pb.close()


# ---- checks 6 and 7
def test_the_same_bits_again_and_for_any_B_and_the_counters(mbavo, gpu_ctx):
    k = 4
    pb, counts, m = _prepared(gpu_ctx, k, k, 0)
    one, c1, _ = _prepared(gpu_ctx, k, k, 0, sel=slice(1, 2))
    try:
        before = pb.stats()
        assert pb.report_stats() == (0, 0, 0)
        a, apc, afl = _report(gpu_ctx, pb)
        stats = pb.report_stats()
        b_, bpc, bfl = _report(gpu_ctx, pb)
        assert bytes(a) == bytes(b_) and np.array_equal(apc, bpc) and np.array_equal(afl, bfl)
        s, spc, sfl = _report(gpu_ctx, one)
        K = int(counts[1, 0])
        assert c1[0, 0] == K and bytes(s[0]) == bytes(a[1]) and np.array_equal(spc[0, :K], apc[1, :K]) and np.array_equal(sfl[0, :K], afl[1, :K])
        launches = _separate_eval(mbavo, gpu_ctx, pb, k)[3]
        assert stats == (launches + 1, 1, B * C.sizeof(mbavo.capi.PairsReport)), (stats, launches)
        assert pb.stats() == before and pb.stats()[3] == _cap0(gpu_ctx, pb)[1]  # the report's scratch is not the plan's
        # the argument rules, nothing launched
        lib, out = gpu_ctx.lib, (mbavo.capi.PairsReport * B)()
        for chi in (-1.0, float("nan"), float("inf")):
            assert lib.mbavo_pairs_report(pb.handle, chi, out, None, None) == E_ARG
        assert lib.mbavo_pairs_report(pb.handle, 3.0, None, None, None) == E_ARG
        assert pb.report_stats() == stats
        fresh = _object(gpu_ctx, k, k)
        try:
            assert lib.mbavo_pairs_report(fresh.handle, 3.0, out, None, None) == E_ARG  # before the first prepare
            c = _case()
            fresh.prepare(*dv.dev(c["sharp"], c["depth"], c["blur"]))
            assert lib.mbavo_pairs_report(fresh.handle, 3.0, out, None, None) == E_ARG  # before the first motion
            assert fresh.report_stats() == (0, 0, 0)
        finally:
            fresh.close()
        plain = pb.report(3.0)  # without the optional arrays
        assert bytes(plain) == bytes(a)
    finally:
        pb.close()
        one.close()


# ---- check 8
def test_a_report_between_lm_and_commit_moves_nothing(mbavo, gpu_ctx):
    """The frame through update, predict, LM, commit on one object and through update, predict, LM, report, commit on its twin: the
    same mbavo_pairs_frame bits, the same state bits; the report itself leaves knots and states as they were."""
    capi, lib = mbavo.capi, gpu_ctx.lib
    n, k = 2, 2
    case = ps.assess_inputs(n, 120, 160, k)
    states = pt.make_states(capi, case)
    from mba_vo_amd import workloads
    make = lambda: workloads.PairBatch(gpu_ctx, n, L=2, H=120, W=160, k=k, N=ps.N_KNOTS, cell=ps.CELL, thresh=ps.THR, border=4)
    plain, with_report = make(), make()
    o = lms.lm_batch_opts(capi, k, 3)
    frames = []
    try:
        sharp, depth, blur = dv.dev(case["sharp"], case["depth"], case["blur"])
        for pb in (plain, with_report):
            pb.prepare(sharp, depth, blur)
            assert pb.set_states(states) == 0
            pb.update(blur)
            assert pb.predict(case["cap"], case["exp"]) == 0
            res = (capi.LmBatchResult * n)()
            assert lib.mbavo_lm_batch_levels(gpu_ctx.handle, n, 2, pb.array, C.byref(o), res, None, 0) == 0
            if pb is with_report:
                kt0, kR0 = pb.knots()
                rep = pb.report(3.0)
                assert all(rep[b].status == 0 and rep[b].num_keypoints0 == pb.array[b * 2].K for b in range(n))
                kt1, kR1 = pb.knots()
                assert np.array_equal(kt0, kt1) and np.array_equal(kR0, kR1)
            frames.append((bytes(pb.commit(ps.FLOW0, ps.FLOW1, ps.KERNEL)), pt.states_bytes(pb.get_states()), pb.track_stats(), pb.step_stats()))
        assert frames[0] == frames[1]
    finally:
        plain.close()
        with_report.close()
