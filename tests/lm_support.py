"""Shared by the LM tests and tools/lm_fuzz.py: the one builder of mbavo_lm_batch_opts, tracking scenes as a B x L problem list
with the run of mbavo_lm_batch_levels on it and the checks of its records against a reference run, the host-loop trackers a
batch of pairs is compared with, and the one-level scenes of tests/test_gpu_lm_batch.py with their host loop."""
import ctypes as C

import numpy as np

import frontend
import tracking
from mba_vo_amd import synth, workloads


def lm_batch_opts(capi, k, max_it, max_nonmono=5, solver=0, sync_every=0, min_q=0.5, min_dec=1e-3, chi=3.0, fast=0.0, groups=0):
    """mbavo_lm_batch_opts; whatever has no argument here stays zero."""
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = k, max_it, max_nonmono
    o.solver_type, o.sync_every, o.fast_solve_ratio, o.groups = solver, sync_every, fast, groups
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = min_q, min_dec, chi
    return o


# ---- tracking scenes over all levels (tests/test_gpu_lm_batch_levels.py)
SOLVE = dict(tracking.OPTS)
CAP = 256


class Pairs:
    """Tracking scenes (tracking.make_tracking_scene, all with the same number of levels) on the device as run_gpu_tracker lays
    them out, as a B x L mbavo_problem list, pair-major: entry b*L + l = pair b at level l, intrinsics of level 0 / 2^l, the
    levels of a pair sharing its capture / exposure times and its knot buffers.  `levels`: which pyramid levels become entries
    (default all; [0]: one-level problems for mbavo_lm_batch)."""

    def __init__(self, mbavo, scenes, levels=None):
        import torch
        from mba_vo_amd.workloads import fill_problem
        capi = mbavo.capi
        dev = "cuda:0"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.scenes = scenes
        nl = len(scenes[0]["levels"])
        self.lv = list(range(nl)) if levels is None else list(levels)
        self.B, self.L = len(scenes), len(self.lv)
        self.array = (capi.Problem * (self.B * self.L))()
        self.keep, self.knots = [], []
        for b, sc in enumerate(scenes):
            assert len(sc["levels"]) == nl
            cap, exp = t(sc["cap"]), t(sc["exp"])
            kt, kR = t(sc["kt0"].ravel()), t(sc["kR0"].ravel())
            start = np.array([int((c - sc["t0"]) / sc["dt"]) for c in sc["cap"]], np.int32)  # tracker.cpp (:549-560)
            self.keep += [cap, exp, start]
            self.knots.append((kt, kR))
            for j, l in enumerate(self.lv):
                lv = sc["levels"][l]
                ref, grad = t(lv["ref"]), t(lv["grad"])
                curs = [t(c) for c in lv["cur"]]
                ptrs = torch.tensor([c.data_ptr() for c in curs], dtype=torch.int64, device=dev)
                xy, z, pat = t(lv["kp_xy"]), t(lv["kp_z"]), t(lv["pattern"])
                self.keep += [ref, grad, curs, ptrs, xy, z, pat]
                # (intrinsics of level 0 / 2^l: tracker.cpp:175)
                fill_problem(self.array[b * self.L + j], lv["S"], sc["F"], lv["kp_xy"].shape[0], lv["pattern"].size // 2, sc["N"], lv["H"], lv["W"],
                             ref, grad, ptrs, xy, z, pat, sc["intr"], cap, exp, sc["t0"], sc["dt"], kt, kR, start, SOLVE["huber_k"], level=l)
        torch.cuda.synchronize()

    def reset(self):
        import torch
        for sc, (kt, kR) in zip(self.scenes, self.knots):
            kt.copy_(torch.from_numpy(sc["kt0"].ravel().copy()))
            kR.copy_(torch.from_numpy(sc["kR0"].ravel().copy()))
        torch.cuda.synchronize()

    def knots_of(self, b):
        kt, kR = self.knots[b]
        return kt.cpu().numpy().reshape(-1, 3), kR.cpu().numpy().reshape(-1, 4)


def levels_opts(mbavo, k, solver=0, fast=0.0, sync_every=3, groups=0, max_it=None):
    """SOLVE's numbers for lm_batch_opts."""
    return lm_batch_opts(mbavo.capi, k, SOLVE["max_num_iterations"] if max_it is None else max_it, SOLVE["max_nonmono"], solver, sync_every,
                         SOLVE["min_step_quality"], SOLVE["min_abs_cost_decrease"], SOLVE["max_chi_square_error"], fast, groups)


def run(mbavo, ctx, pairs, o, levels=True):
    """One call (mbavo_lm_batch_levels, or mbavo_lm_batch for levels=False) from the initial knots: per pair (result, records, knots)."""
    import torch
    capi = mbavo.capi
    pairs.reset()
    B = pairs.B
    res = (capi.LmBatchResult * B)()
    trace = (capi.TraceRec * (B * CAP))()
    if levels:
        rc = ctx.lib.mbavo_lm_batch_levels(ctx.handle, B, pairs.L, pairs.array, C.byref(o), res, trace, CAP)
    else:
        rc = ctx.lib.mbavo_lm_batch(ctx.handle, B, pairs.array, C.byref(o), res, trace, CAP)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = []
    for b in range(B):
        r = res[b]
        assert 0 < r.num_trace <= CAP, r.num_trace
        recs = [(t.level, t.iter, t.kind, t.num_outliers, t.radius, t.eval_cost, t.candidate_cost, t.model_change, t.quality)
                for t in trace[b * CAP:b * CAP + r.num_trace]]
        fields = (r.iterations, r.accepted, r.rejected, r.invalid, r.num_outliers, r.num_trace, r.initial_cost, r.final_cost, r.radius)
        out.append((fields, recs, pairs.knots_of(b)))
    return out


def per_level_iterations(recs):
    """n_{b,l}: the iterations of each level (a level's records end with its last iteration's)."""
    n = {}
    for r in recs:
        n[r[0]] = max(n.get(r[0], 0), r[1])
    return n


def flip_margin(a, b):
    """Where two record sequences first part: the accept test's margins there (quality - min_q, eval - candidate cost)."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x[:4] != y[:4]:
            return "record %d: %s vs %s; quality - min_q %.3e / %.3e, eval - cand %.3e / %.3e" % (
                i, x[:4], y[:4], x[8] - SOLVE["min_step_quality"], y[8] - SOLVE["min_step_quality"], x[5] - x[6], y[5] - y[6])
    return "lengths %d vs %d" % (len(a), len(b))


def check_against(got, want, want_kt, want_kR, want_cost, tag):
    fields, recs, (kt, kR) = got
    assert [r[:4] for r in recs] == [r[:4] for r in want], (tag, flip_margin(recs, want))
    for d, h in zip(recs, want):
        assert abs(d[4] - h[4]) <= 1e-4 * h[4], (tag, d, h)                         # radius
        for i in (5, 6, 7):                                                          # costs, model change
            assert abs(d[i] - h[i]) <= 1e-5 * max(1.0, abs(h[i])), (tag, i, d, h)
        assert abs(d[8] - h[8]) <= 1e-3 * max(1.0, abs(h[8])), (tag, d, h)          # quality
    assert abs(fields[7] - want_cost) <= 1e-5 * max(1.0, want_cost), (tag, fields[7], want_cost)
    assert np.abs(kt - want_kt).max() < 1e-4 and np.abs(kR - want_kR).max() < 1e-4, tag


def check_fields(got, L):
    """The result fields against the pair's own records: sums over the levels, initial cost of the coarsest level's iteration 0,
    final cost / radius / outliers as level 0 ends."""
    (iterations, accepted, rejected, invalid, num_outliers, num_trace, initial, final, radius), recs, _ = got
    n = per_level_iterations(recs)
    assert sorted(n) == list(range(L)) and [r[0] for r in recs] == sorted((r[0] for r in recs), reverse=True)
    assert iterations == sum(n.values()) and num_trace == len(recs)
    assert accepted == sum(r[2] == 1 for r in recs) and rejected == sum(r[2] == 2 for r in recs) and invalid == sum(r[2] == 3 for r in recs)
    assert recs[0][:3] == (L - 1, 0, 0) and initial == recs[0][5]
    assert recs[-1][0] == 0 and final == recs[-1][5] and radius == recs[-1][4] and num_outliers == recs[-1][3]
    assert sum(r[2] == 0 for r in recs) == L and all(r[1] == 0 for r in recs if r[2] == 0)


# ---- host-loop trackers (tests/test_gpu_pairs_step.py, tests/test_gpu_pairs_track.py)
def run_trackers(mbavo, ctx, seqs, cfg):
    """Six free-running mbavo_vo trackers, as frontend.run_gpu_vo runs one, with mbavo_vo_get_state before every frame and the
    index of the frame whose sharp image is the keyframe at that time."""
    capi = mbavo.capi
    runs = []
    for seq in seqs:
        o, keep = frontend.fill_gpu_opts(capi, seq, cfg)
        vo = capi.vp()
        capi.check(ctx.lib.mbavo_vo_create(ctx.handle, C.byref(o), C.byref(vo)), "mbavo_vo_create")
        recs = (capi.TraceRec * frontend.TRACE_CAP)()
        out, kf_index = [], 0
        try:
            for i, t in enumerate(seq["times"]):
                st, T, info = capi.VoState(), np.zeros(7), capi.VoInfo()
                capi.check(ctx.lib.mbavo_vo_get_state(vo, C.byref(st)), "mbavo_vo_get_state")
                rc = ctx.lib.mbavo_vo_track_frame(vo, seq["sharp"][i].ctypes.data, seq["depth"][i].ctypes.data, float(t), seq["blur"][i].ctypes.data,
                                                  float(t), float(seq["exp"]), capi.dp(T), C.byref(info))
                assert rc == 0, rc
                nst = capi.VoState()
                capi.check(ctx.lib.mbavo_vo_get_state(vo, C.byref(nst)), "mbavo_vo_get_state")
                out.append(dict(state=st, state_after=nst, kf=kf_index, T=T, is_keyframe=info.is_keyframe, avg_flow=info.avg_flow,
                                avg_kernel=info.avg_kernel, cost=info.final_cost, K0=info.num_keypoints0,
                                trace=frontend._trace_rows(recs, ctx.lib.mbavo_vo_last_trace(vo, recs, frontend.TRACE_CAP)) if i else []))
                if info.is_keyframe:
                    kf_index = i
        finally:
            ctx.lib.mbavo_vo_destroy(vo)
        runs.append(out)
    return runs


# ---- one-level scenes (tests/test_gpu_lm_batch.py, tools/lm_fuzz.py)
OPTS = dict(max_it=25, max_nonmono=5, min_q=0.5, min_dec=1e-3, chi=3.0)


def scene(B, k, N, F, seed, H=96, W=128, S=4, kR=None):
    """B independent pairs with their own splines; F frames per pair at different knot segments.  kR: a function b -> rotation
    knots [N, 4] that replaces pair b's (default: the harness spline's at rot_scale = 0.05)."""
    rng = np.random.default_rng(seed)
    probs = []
    ref0 = synth.texture_image(H, W, seed=seed, octaves=(32, 16, 8, 4))
    grad0 = synth.image_gradients(ref0)
    xy, z = synth.semi_dense_keypoints(ref0, cell=10, thresh=2.0, margin=8, seed=seed + 1)
    intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
    t0, dt = 0.0, 0.5
    cap = [0.25 + 0.5 * f for f in range(F)]
    exp = [0.1] * F
    assert int((cap[-1] + exp[-1]) / dt) + k <= N
    for b in range(B):
        kt, kR_b = synth.harness_spline(0.004, 0.05, N)
        if kR is not None:
            kR_b = np.ascontiguousarray(kR(b), np.float64).reshape(N, 4)
        kt = kt + rng.normal(0, 2e-3, kt.shape)
        curs = [workloads._current_image(ref0, rng, shift=(1 + (b + f) % 2, -(1 + b % 2)), noise=3) for f in range(F)]
        probs.append(workloads.Prob(ref0, curs, xy, z, synth.PATTERN8, intr, S, k, N, cap, exp, t0, dt, kt, kR_b, 10.0, grad=grad0))
    return probs


def host_lm(mbavo, ctx, dw, b, p, solver, trace_cap=64, fast_solve_ratio=0.0):
    capi = mbavo.capi
    lv = (capi.Level * 1)()
    q, a = lv[0], dw.array[b]
    q.H, q.W, q.K, q.P, q.S = p.H, p.W, p.K, p.P, p.S
    q.d_ref_img, q.d_ref_dIxy, q.d_cur_imgs = a.d_ref_img, a.d_ref_dIxy, a.d_cur_imgs
    q.d_kp_xy, q.d_kp_z, q.d_pattern = a.d_kp_xy, a.d_kp_z, a.d_pattern
    o = capi.TrackOpts()
    o.num_levels, o.spline_deg_k, o.max_num_iterations = 1, p.k, OPTS["max_it"]
    o.max_consecutive_nonmonotonic_steps, o.solver_type = OPTS["max_nonmono"], solver
    for i in range(4):
        o.intrinsics[i] = float(p.intr[i])
    o.huber_k, o.min_step_quality = p.huber, OPTS["min_q"]
    o.min_abs_cost_decrease, o.max_chi_square_error = OPTS["min_dec"], OPTS["chi"]
    o.fast_solve_ratio = fast_solve_ratio  # (0: the default stand-in up to a pivot ratio of 1e8; -1: the reference's solvers for every system)
    kt, kR = p.knots_t.copy(), p.knots_R.copy()
    start, cost = np.zeros(p.F, np.int32), np.zeros(1)
    trace = (capi.TraceRec * trace_cap)()
    n = ctx.lib.mbavo_optimize_trajectory(ctx.handle, C.byref(o), lv, p.F, capi.dp(p.cap), capi.dp(p.exp), p.t0, p.dt,
                                          capi.dp(kt), capi.dp(kR), p.N, capi.ip(start), capi.dp(cost), trace, trace_cap)
    assert 0 < n <= trace_cap, n
    return kt, kR, float(cost[0]), [(r.iter, r.kind, r.num_outliers, r.radius, r.eval_cost, r.candidate_cost, r.model_change, r.quality)
                                    for r in trace[:n]]


# ---- what a call leaves behind on its context (tests/test_gpu_lm_batch.py, tests/test_gpu_segment_range.py)
def reset_knots(dw, probs):
    import torch
    for b, p in enumerate(probs):
        dw.keep_knots(b)[0].copy_(torch.from_numpy(p.knots_t))
        dw.keep_knots(b)[1].copy_(torch.from_numpy(p.knots_R))
    torch.cuda.synchronize()


def lm_bits(capi, ctx, dw, probs, o, cap=48):
    """One mbavo_lm_batch from the initial knots: (rc, every result field, the whole trace buffer, the final knots) as bytes."""
    import torch
    B = len(probs)
    reset_knots(dw, probs)
    res = (capi.LmBatchResult * B)()
    trace = (capi.TraceRec * (B * cap))()
    rc = ctx.lib.mbavo_lm_batch(ctx.handle, B, dw.array, C.byref(o), res, trace, cap)
    torch.cuda.synchronize()
    knots = b"".join(x.cpu().numpy().tobytes() for b in range(B) for x in dw.keep_knots(b))
    return rc, bytes(res), bytes(trace), knots, sum(r.accepted for r in res)


def eval_bits(ctx, dw, probs):
    """One mbavo_eval_batch (H / g) at the initial knots: the packed frame blocks as bytes."""
    import torch
    reset_knots(dw, probs)
    dw.frame_blocks.zero_()
    dw.step(ctx, with_hessian=True, merged=False)
    torch.cuda.synchronize()
    return dw.frame_blocks.cpu().numpy().tobytes()
