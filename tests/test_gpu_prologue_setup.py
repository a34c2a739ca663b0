"""-m gpu: the set-up and the hand-over of the lane-per-pixel kernel's pose prologue (engine.hip: k_fused<.., POSE>, fused_setup).

The waves of a workgroup that take no part in the prologue's two stages work out the pose-independent set-up (sample-count
constants, reciprocal intrinsics, residual scale, the split of the tile into lane-per-pixel rounds and a sample-parallel remainder)
BEFORE they wait at its barrier, the others behind it, and the vector warm-up read of the freshly written table lines is gone.  None
of that touches an arithmetic instruction, so every output must be the SAME BITS as with the pose kernel ahead (fused_pose = -1),
which runs the same set-up in its one place; the oracle bounds are the project's (test_gpu_fuzz._tol).

Shapes: the smallest at which this code can go wrong -- dense one-pixel patches at 64x48 and 32x24 in one batch (a few tiles, fewer
than there are CUs, so the prologue form is chosen: asserted through mbavo_last_kernel / mbavo_last_layout), k = 2 and 4, H/g and
cost-only, S = 1, 8, 21 and a batch that mixes S = 4 with S = 8 (table_stride is the larger); one-tile problems whose pixel counts
hit every branch of the remainder decision (npx % 256 = 0, 1, 255, a tile smaller than one round); and knots rewritten in place
between calls on one engine (A, B, A: the scalar cache must not serve the previous call's entries).

A problem whose `active` word is cleared returns ahead of the prologue's barriers.  The C ABI sets that word inside mbavo_lm_batch
only (a pair that has finished sits the later passes out), so that case runs a small batch through mbavo_lm_batch with the
evaluations' own pose entries (pose_entries = -1), once with the prologue and once with the pose kernel ahead: pairs finish at
different iterations, the passes of the later ones run k_fused<.., POSE> beside workgroups that left early, and every record,
result and final knot must be the same bits."""
import ctypes as C

import numpy as np
import pytest

import eval_support as es
import lm_support as lms
import scenes

pytestmark = pytest.mark.gpu

PROLOGUE = dict(sample_parallel=-1, fused_pose=1, fused_pose_max_samples=21)
POSE_KERNEL = dict(sample_parallel=-1, fused_pose=-1, fused_pose_max_samples=21)
BITS = ("fb", "pc", "valid", "fc", "pcc", "validc", "fb_m", "sys_m", "sys_a")


def _dense(H, W, S, k, seed):
    return dict(H=H, W=W, S=S, F=1, k=k, P=1, kp="dense", margin=0, seed=seed)


def _one_tile(K, S, k, seed):
    # K one-pixel patches in one tile (min_tile_pixels far above K): npx = K
    return dict(H=120, W=160, S=S, F=1, k=k, P=1, K=K, margin=12, seed=seed)


# name -> (k, scene keywords, extra engine options)
LISTS = {}
for _k in (2, 4):
    for _S in (1, 8, 21):
        LISTS["dense_k%d_S%d" % (_k, _S)] = (_k, [_dense(48, 64, _S, _k, 100 + _S), _dense(24, 32, _S, _k, 200 + _S)], {})
    LISTS["dense_k%d_S4_S8" % _k] = (_k, [_dense(48, 64, 4, _k, 301), _dense(24, 32, 8, _k, 302), _dense(24, 32, 4, _k, 303)], {})
    # the remainder decision of fused_setup: npx % 256 = 0 (no remainder), 1 and 255 (sample-parallel remainder: 1 << 2 lanes per
    # pixel fit the workgroup or do not), a tile smaller than a round (all of it remainder, or one partial round)
    for _K in (512, 257, 511, 40, 1):
        LISTS["tile_k%d_K%d" % (_k, _K)] = (_k, [_one_tile(_K, 8, _k, 400 + _K)], dict(min_tile_pixels=1 << 20))
    LISTS["tile_k%d_K255_S4" % _k] = (_k, [_one_tile(255, 4, _k, 450)], dict(min_tile_pixels=1 << 20))

_DATA = {}


def _data(orc, name):
    """Scenes, device twins and oracle results of one list: once, shared and never modified."""
    if name not in _DATA:
        k, kws, _ = LISTS[name]
        scs = [scenes.Scene(**kw) for kw in kws]
        ds = [scenes.DeviceScene(sc) for sc in scs]
        oracle = []
        for sc in scs:
            p, keep = sc.oracle_problem(orc)
            ro, roc = orc.evaluate(p), orc.evaluate(p, with_hessian=False)
            want = (ro["frame_blocks"].reshape(sc.F, sc.E).copy(), roc["frame_blocks"].reshape(sc.F, sc.E)[:, 0].copy(),
                    es.oracle_valid_counts(orc, sc))
            for a in want:
                a.setflags(write=False)
            oracle.append(want)
        _DATA[name] = (scs, ds, oracle)
    return _DATA[name]


def _both_forms(mbavo, ctx, k, scs, ds, extra):
    runs = {}
    try:
        for form, opts in (("prologue", PROLOGUE), ("pose_kernel", POSE_KERNEL)):
            ctx.engine_opts(**dict(opts, **extra))
            runs[form] = es.run(mbavo, ctx, k, scs, ds)
    finally:
        ctx.engine_opts()
    return runs["prologue"], runs["pose_kernel"]


def _witness(f, p, k, scs):
    """The prologue form was chosen (no more tiles than CUs, lane-per-pixel kernel) and the other run had the pose kernel ahead."""
    for kern, with_h in ((f["kern"], "true"), (f["kern_c"], "false"), (f["kern_m"], "true")):
        assert kern == "k_fused<%d,%s,false,true>" % (k, with_h), kern
    assert p["kern"] == "k_fused<%d,true,false,false>" % k and p["kern_c"] == "k_fused<%d,false,false,false>" % k, (p["kern"], p["kern_c"])
    assert es.per_pixel_kernel(f["kern"]) == es.per_pixel_kernel(p["kern"])
    for lay in (f["lay"], f["lay_c"], f["lay_m"]):
        assert 0 < lay["ntiles"] <= lay["num_cus"] and lay["sp_logs"] == 0 and lay["empty"] == 0 and lay["nprob"] == len(scs), lay
    assert f["lay"] == p["lay"]


@pytest.mark.parametrize("name", list(LISTS))
def test_prologue_setup_same_bits_as_pose_kernel(orc, mbavo, gpu_ctx, name):
    k, kws, extra = LISTS[name]
    scs, ds, oracle = _data(orc, name)
    f, p = _both_forms(mbavo, gpu_ctx, k, scs, ds, extra)
    _witness(f, p, k, scs)
    if name.startswith("tile_"):
        assert f["lay"]["ntiles"] == 1 and scs[0].K * scs[0].P == kws[0]["K"], f["lay"]
    for key in BITS:
        assert np.array_equal(f[key], p[key]), (name, key)
    assert np.array_equal(f["fb_m"], f["fb"]) and np.array_equal(f["sys_m"], f["sys_a"])
    row = 0
    for sc, (fbo, fco, vo) in zip(scs, oracle):
        rows = slice(row, row + sc.F)
        row += sc.F
        tol = es.tol(sc)
        d_fb = np.abs(f["fb"][rows] - fbo).max() / np.abs(fbo).max()
        d_fc = np.abs(f["fc"][rows] - fco).max() / max(np.abs(fco).max(), 1e-300)
        print("prologue_setup_figures %s S=%d K=%d fb=%.3g fc=%.3g tol=%.3g" % (name, sc.S, sc.K, d_fb, d_fc, tol))
        assert d_fb <= tol and d_fc <= tol, (name, d_fb, d_fc, tol)
        assert np.array_equal(f["valid"][rows], vo) and np.array_equal(f["validc"][rows], vo)


def test_remainder_branches_are_reached():
    """The one-tile cases cover npx % 256 = 0, 1, 255 and a tile below one round, for both workgroup sizes (k = 2: 1024, k = 4: 768
    threads; cost-only k = 4: 1024), with S = 8 (two samples per lane in the remainder) and S = 4 (one)."""
    for k in (2, 4):
        Ks = sorted(kws[0]["K"] for n, (kk, kws, _) in LISTS.items() if n.startswith("tile_k%d" % k))
        assert {K % 256 for K in Ks} >= {0, 1, 255} and min(Ks) < 64 and any(K < 256 for K in Ks), Ks


@pytest.mark.parametrize("k", [2, 4])
def test_knots_rewritten_in_place_between_calls(orc, mbavo, gpu_ctx, k):
    """One engine, one problem list, the same table addresses: knots A, then B, then A again written into the SAME device arrays.
    Call 3 equals call 1 bit for bit and call 2 equals a fresh engine's evaluation of B -- a hand-over that let the scalar cache (or
    the L2 of another launch) serve the previous call's entries would fail either."""
    import torch
    scs = [scenes.Scene(**_dense(48, 64, 8, k, 501)), scenes.Scene(**_dense(24, 32, 8, k, 502))]
    ds = [scenes.DeviceScene(sc) for sc in scs]
    # (the harness spline's rotation knots depend on the scales alone: B gets other ones)
    others = [scenes.Scene(trans_scale=0.006, rot_scale=0.03, **_dense(48, 64, 8, k, 503)),
              scenes.Scene(trans_scale=0.006, rot_scale=0.03, **_dense(24, 32, 8, k, 504))]
    knots = {"A": [(torch.from_numpy(sc.knots_t).cuda(), torch.from_numpy(sc.knots_R).cuda()) for sc in scs],
             "B": [(torch.from_numpy(o.knots_t).cuda(), torch.from_numpy(o.knots_R).cuda()) for o in others]}
    for sc, o in zip(scs, others):
        assert sc.N == o.N and not np.array_equal(sc.knots_R, o.knots_R)

    def put(which):
        for d, (kt, kR) in zip(ds, knots[which]):
            d.knots_t.copy_(kt)
            d.knots_R.copy_(kR)
        torch.cuda.synchronize()

    calls = []
    try:
        gpu_ctx.engine_opts(**PROLOGUE)
        for which in "ABA":
            put(which)
            calls.append(es.run(mbavo, gpu_ctx, k, scs, ds))
    finally:
        gpu_ctx.engine_opts()
    fresh_ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        put("B")
        fresh_ctx.engine_opts(**PROLOGUE)
        fresh = es.run(mbavo, fresh_ctx, k, scs, ds)
    finally:
        fresh_ctx.close()
        put("A")
    for c in calls + [fresh]:
        assert c["kern"] == "k_fused<%d,true,false,true>" % k and c["kern_c"] == "k_fused<%d,false,false,true>" % k, c["kern"]
    for key in BITS:
        assert np.array_equal(calls[2][key], calls[0][key]), ("A again", key)
        assert np.array_equal(calls[1][key], fresh[key]), ("B", key)
    assert not np.array_equal(calls[0]["fb"], calls[1]["fb"])  # the two sets of knots do give different results


LM_CASES = [(4, 6, 1, 4), (4, 4, 1, 8), (2, 4, 2, 4)]


@pytest.mark.parametrize("k,N,F,S", LM_CASES, ids=["k%d-N%d-F%d-S%d" % c for c in LM_CASES])
def test_inactive_problems_leave_ahead_of_the_prologue(mbavo, gpu_ctx, k, N, F, S):
    """mbavo_lm_batch over 12 pairs whose evaluations make their own pose entries: with fused_pose = 1 every pass is
    k_fused<k, .., POSE> (witness: the call's last evaluation), with fused_pose = -1 the pose kernel runs ahead.  The pairs finish
    after different numbers of iterations, so the passes of the later ones hold workgroups whose problem has `active` cleared: they
    return before the prologue's first barrier and leave their outputs alone.  Trace records, results and final knots are identical
    bit for bit between the two forms, and steps are taken."""
    import torch
    from mba_vo_amd import workloads
    capi = mbavo.capi
    out, kern = {}, {}
    try:
        for fp in (1, -1):
            gpu_ctx.engine_opts(sample_parallel=-1, fused_pose=fp)
            probs = lms.scene(12, k, N, F, seed=43, S=S)
            dw = workloads.DeviceWorkload(probs)
            o = lms.lm_batch_opts(capi, k, **dict(lms.OPTS, max_it=12))
            o.pose_entries = -1
            B, cap = len(probs), 32
            res = (capi.LmBatchResult * B)()
            trace = (capi.TraceRec * (B * cap))()
            assert gpu_ctx.lib.mbavo_lm_batch(gpu_ctx.handle, B, dw.array, C.byref(o), res, trace, cap) == 0
            torch.cuda.synchronize()
            kern[fp], lay = gpu_ctx.lib.mbavo_last_kernel(gpu_ctx.handle).decode(), es.layout(gpu_ctx)
            assert 0 < lay["ntiles"] <= lay["num_cus"] and lay["sp_logs"] == 0 and lay["nprob"] == B, lay
            recs = [[(t.iter, t.kind, t.num_outliers, t.radius, t.eval_cost, t.candidate_cost, t.model_change, t.quality)
                     for t in trace[b * cap:b * cap + res[b].num_trace]] for b in range(B)]
            knots = [tuple(x.cpu().numpy().tobytes() for x in dw.keep_knots(b)) for b in range(B)]
            out[fp] = (recs, knots, [(r.iterations, r.accepted, r.rejected, r.invalid, r.final_cost) for r in res])
    finally:
        gpu_ctx.engine_opts()
    print("prologue_setup_lm k=%d kernels %s iterations %s" % (k, kern, [r[0] for r in out[1][2]]))
    assert kern[1].startswith("k_fused<%d," % k) and kern[1].endswith(",true>"), kern
    assert kern[-1].startswith("k_fused<%d," % k) and kern[-1].endswith(",false>"), kern
    iters = [r[0] for r in out[1][2]]
    assert min(iters) < max(iters), iters  # some pairs sat passes out while others ran
    assert sum(r[1] for r in out[1][2]) > 0  # steps were taken
    assert repr(out[1]) == repr(out[-1]), (k, N, F, S)
