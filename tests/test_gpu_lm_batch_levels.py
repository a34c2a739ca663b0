"""Device-side batched LM over all pyramid levels (mbavo_lm_batch_levels): B pairs, each aligned coarse to fine as
optimizeTrajectory does (blur_aware_direct_tracker.cpp:544-588), in one call.  Held against the host-driven loop
(mbavo_optimize_trajectory, pair after pair) and the oracle with the tolerances of tests/test_gpu_lm_batch.py: the (level,
iteration, kind, outlier count) sequence exact; costs 1e-5 relative, radius 1e-4, quality 1e-3, knots 1e-4 absolute.  L = 1 is
mbavo_lm_batch bit for bit; the schedules (sync_every, groups) give the same bits; a pair goes on to its next level without
waiting for the others."""
import ctypes as C
import re

import numpy as np
import pytest

import tracking

pytestmark = pytest.mark.gpu

SOLVE = dict(tracking.OPTS)
CAP = 256


class _Pairs:
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


def _opts(mbavo, k, solver=0, fast=0.0, sync_every=3, groups=0, max_it=None):
    o = mbavo.capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations = k, SOLVE["max_num_iterations"] if max_it is None else max_it
    o.max_consecutive_nonmonotonic_steps, o.solver_type, o.sync_every = SOLVE["max_nonmono"], solver, sync_every
    o.min_step_quality, o.min_abs_cost_decrease = SOLVE["min_step_quality"], SOLVE["min_abs_cost_decrease"]
    o.max_chi_square_error, o.fast_solve_ratio, o.groups = SOLVE["max_chi_square_error"], fast, groups
    return o


def _run(mbavo, ctx, pairs, o, levels=True):
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


def _per_level_iterations(recs):
    """n_{b,l}: the iterations of each level (a level's records end with its last iteration's)."""
    n = {}
    for r in recs:
        n[r[0]] = max(n.get(r[0], 0), r[1])
    return n


def _flip_margin(a, b):
    """Where two record sequences first part: the accept test's margins there (quality - min_q, eval - candidate cost)."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x[:4] != y[:4]:
            return "record %d: %s vs %s; quality - min_q %.3e / %.3e, eval - cand %.3e / %.3e" % (
                i, x[:4], y[:4], x[8] - SOLVE["min_step_quality"], y[8] - SOLVE["min_step_quality"], x[5] - x[6], y[5] - y[6])
    return "lengths %d vs %d" % (len(a), len(b))


def _check_against(got, want, want_kt, want_kR, want_cost, tag):
    fields, recs, (kt, kR) = got
    assert [r[:4] for r in recs] == [r[:4] for r in want], (tag, _flip_margin(recs, want))
    for d, h in zip(recs, want):
        assert abs(d[4] - h[4]) <= 1e-4 * h[4], (tag, d, h)                         # radius
        for i in (5, 6, 7):                                                          # costs, model change
            assert abs(d[i] - h[i]) <= 1e-5 * max(1.0, abs(h[i])), (tag, i, d, h)
        assert abs(d[8] - h[8]) <= 1e-3 * max(1.0, abs(h[8])), (tag, d, h)          # quality
    assert abs(fields[7] - want_cost) <= 1e-5 * max(1.0, want_cost), (tag, fields[7], want_cost)
    assert np.abs(kt - want_kt).max() < 1e-4 and np.abs(kR - want_kR).max() < 1e-4, tag


def _check_fields(got, L):
    """The result fields against the pair's own records: sums over the levels, initial cost of the coarsest level's iteration 0,
    final cost / radius / outliers as level 0 ends."""
    (iterations, accepted, rejected, invalid, num_outliers, num_trace, initial, final, radius), recs, _ = got
    n = _per_level_iterations(recs)
    assert sorted(n) == list(range(L)) and [r[0] for r in recs] == sorted((r[0] for r in recs), reverse=True)
    assert iterations == sum(n.values()) and num_trace == len(recs)
    assert accepted == sum(r[2] == 1 for r in recs) and rejected == sum(r[2] == 2 for r in recs) and invalid == sum(r[2] == 3 for r in recs)
    assert recs[0][:3] == (L - 1, 0, 0) and initial == recs[0][5]
    assert recs[-1][0] == 0 and final == recs[-1][5] and radius == recs[-1][4] and num_outliers == recs[-1][3]
    assert sum(r[2] == 0 for r in recs) == L and all(r[1] == 0 for r in recs if r[2] == 0)


def _scenes(orc, k, seeds, sizes=((120, 160), (240, 320)), frames=(1, 2)):
    return [tracking.make_tracking_scene(orc, H=sizes[i % len(sizes)][0], W=sizes[i % len(sizes)][1], levels=3, S=8, k=k,
                                         F=frames[(i // len(sizes)) % len(frames)], seed=s)
            for i, s in enumerate(seeds)]


@pytest.mark.parametrize("k,solver,fast", [(4, 0, 0.0), (4, 0, -1.0), (2, 0, 0.0), (4, 1, 0.0), (2, 1, -1.0)])
def test_levels_match_host_loop(orc, mbavo, gpu_ctx, k, solver, fast):
    """B = 6 pairs (120 x 160 and 240 x 320, F = 1 and 2, 3 levels) in one call against mbavo_optimize_trajectory per pair with
    the same options: the record sequence (level, iteration, kind, outliers) identical, values and knots to the stated tolerances,
    the result fields consistent with the records."""
    scs = _scenes(orc, k, seeds=[31 + 10 * k + i for i in range(6)])
    opts = dict(SOLVE, solver_type=solver, fast_solve_ratio=fast)
    host = [tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, opts) for sc in scs]
    pairs = _Pairs(mbavo, scs)
    got = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, k, solver, fast))
    kinds = set()
    for b, (g, h) in enumerate(zip(got, host)):
        _check_against(g, h["trace"], h["kt"], h["kR"], h["cost"], (k, solver, fast, b))
        _check_fields(g, 3)
        kinds |= {r[2] for r in g[1]}
        assert np.abs(g[2][0] - scs[b]["kt0"]).max() > 1e-9  # the knots really moved
    assert 1 in kinds and 2 in kinds


def test_levels_against_oracle(orc, mbavo, gpu_ctx):
    """A few pairs against the oracle's optimizeTrajectory (tracking.run_oracle_tracker), same rules."""
    for k in (4, 2):
        scs = _scenes(orc, k, seeds=[70 + k, 71 + k, 72 + k])
        want = [tracking.run_oracle_tracker(orc, sc, SOLVE) for sc in scs]
        got = _run(mbavo, gpu_ctx, _Pairs(mbavo, scs), _opts(mbavo, k, sync_every=0))
        for b, (g, w) in enumerate(zip(got, want)):
            _check_against(g, w["trace"], w["kt"], w["kR"], w["cost"], (k, b))
            _check_fields(g, 3)


def test_one_level_is_lm_batch(orc, mbavo, gpu_ctx):
    """L = 1 through the new entry and mbavo_lm_batch on the same one-level problems (each scene's level 0 and, as a second
    batch, its level 1): identical bits -- every record field, the result fields, the knots -- for sync_every 0 and 3."""
    scs = _scenes(orc, 4, seeds=[90, 91, 92, 93])
    for lv in (0, 1):
        pairs = _Pairs(mbavo, scs, levels=[lv])
        for se in (0, 3):
            a = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=se), levels=True)
            b = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=se), levels=False)
            assert repr([(x[0], x[1]) for x in a]) == repr([(x[0], x[1]) for x in b]), (lv, se)
            for x, y in zip(a, b):
                assert np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1]), (lv, se)
            assert all(r[0] == 0 for x in a for r in x[1])  # (one level: the records say level 0, as mbavo_lm_batch's)


def test_levels_schedules_same_bits(orc, mbavo, gpu_ctx):
    """The schedule changes nothing: sync_every 0 (pinned words, look-ahead) and 3 (stream drains) give identical records, result
    fields and knots.  So does the batch split into two groups on their own engines and streams (groups = 2, at a pair boundary)
    where both groups' lists take the same evaluation kernel as the whole list (mbavo_engine_opts.sample_parallel = -1: the
    lane-per-pixel kernel, every entry's tiles within the tile target either way).  With the defaults a half list may take the
    sample-parallel kernel where the whole does not: other sums, the last bits of the values differ -- the discrete records do not."""
    import torch
    scs = _scenes(orc, 4, seeds=[110 + i for i in range(6)])
    pairs = _Pairs(mbavo, scs)

    def same_bits(got, base, tag):
        assert repr([(x[0], x[1]) for x in got]) == repr([(x[0], x[1]) for x in base]), tag
        for x, y in zip(got, base):
            assert np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1]), tag

    base = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=0))
    same_bits(_run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=3)), base, "sync_every")
    got = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=0, groups=2))
    assert [[r[:4] for r in x[1]] for x in got] == [[r[:4] for r in x[1]] for x in base]
    assert sum(x[0][1] for x in base) > 0
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.engine_opts(sample_parallel=-1)
        one = _run(mbavo, ctx, pairs, _opts(mbavo, 4, sync_every=0))
        for kw in (dict(sync_every=0, groups=2), dict(sync_every=3, groups=2)):
            same_bits(_run(mbavo, ctx, pairs, _opts(mbavo, 4, **kw)), one, kw)
    finally:
        ctx.close()


def test_pairs_do_not_wait_for_each_other(orc, mbavo, gpu_ctx, capfd, monkeypatch):
    """A pair moves on to its next level in the slot its current level ends: the call takes at most max_b sum_l (n_{b,l} + 2)
    slots (n_{b,l}: pair b's iterations on level l, from its records), while levels in lock-step would take at least
    sum_l max_b n_{b,l}.  The batch is built from the records of a pool of pairs so that the two bounds differ: for every level
    the pair with the most iterations there, filled up with the pairs of the fewest iterations in all.  Slots are counted from the
    per-slot lines MBAVO_LM_STAMPS=1 prints (default sync_every).  The pool: 16 pairs (120 x 160 and 240 x 320) with initial knots
    5x further off than the default (perturb 2e-2), so that the coarse levels have work too."""
    pool_sc = [tracking.make_tracking_scene(orc, H=H, W=W, levels=3, S=8, k=4, F=1, seed=130 + i, perturb=2e-2)
               for (H, W) in ((120, 160), (240, 320)) for i in range(8)]
    pool = _run(mbavo, gpu_ctx, _Pairs(mbavo, pool_sc), _opts(mbavo, 4, sync_every=3))
    n = [_per_level_iterations(x[1]) for x in pool]
    pick = []
    for l in range(3):
        b = max(range(len(n)), key=lambda i: (n[i][l] - sum(n[i][m] for m in range(3) if m != l), -i))
        if b not in pick:
            pick.append(b)
    for b in sorted(range(len(n)), key=lambda i: (sum(n[i].values()), i)):
        if len(pick) >= 8:
            break
        if b not in pick:
            pick.append(b)
    pairs = _Pairs(mbavo, [pool_sc[b] for b in pick])
    monkeypatch.setenv("MBAVO_LM_STAMPS", "1")
    capfd.readouterr()
    got = _run(mbavo, gpu_ctx, pairs, _opts(mbavo, 4, sync_every=0))
    err = capfd.readouterr().err
    monkeypatch.delenv("MBAVO_LM_STAMPS")
    slots = len(re.findall(r"^mbavo lm_batch:\s+slot \d+:", err, re.M))
    nb = [_per_level_iterations(x[1]) for x in got]
    bound = max(sum(v + 2 for v in m.values()) for m in nb)
    lock_step = sum(max(m[l] for m in nb) for l in range(3))
    assert bound < lock_step, (nb, bound, lock_step)  # (a precondition of the batch)
    assert 0 < slots <= bound, (slots, bound, lock_step, nb)


def test_levels_argument_errors(orc, mbavo, gpu_ctx):
    """MBAVO_E_ARG (-1) with nothing launched: knot buffers that differ within a pair, L = 0, L = 9, a null problem list, a level
    with another capture-time buffer; the context works afterwards."""
    capi = mbavo.capi
    scs = _scenes(orc, 4, seeds=[150, 151])
    pairs = _Pairs(mbavo, scs)
    o = _opts(mbavo, 4)
    res = (capi.LmBatchResult * 2)()
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good = _run(mbavo, gpu_ctx, pairs, o)
    pairs.reset()
    a = pairs.array
    keep = a[1].d_knots_t
    a[1].d_knots_t = a[4].d_knots_t  # pair 0, level 1: pair 1's knots
    assert lib.mbavo_lm_batch_levels(h, 2, 3, a, C.byref(o), res, None, 0) == -1
    a[1].d_knots_t = keep
    keep = a[5].d_cap_time
    a[5].d_cap_time = a[0].d_cap_time
    assert lib.mbavo_lm_batch_levels(h, 2, 3, a, C.byref(o), res, None, 0) == -1
    a[5].d_cap_time = keep
    assert lib.mbavo_lm_batch_levels(h, 2, 0, a, C.byref(o), res, None, 0) == -1
    assert lib.mbavo_lm_batch_levels(h, 1, 9, a, C.byref(o), res, None, 0) == -1
    assert lib.mbavo_lm_batch_levels(h, 2, 3, None, C.byref(o), res, None, 0) == -1
    for x, y in zip(pairs.knots, scs):  # nothing ran: the knots are the initial ones
        assert np.array_equal(x[0].cpu().numpy(), y["kt0"].ravel())
    again = _run(mbavo, gpu_ctx, pairs, o)
    assert repr([(x[0], x[1]) for x in again]) == repr([(x[0], x[1]) for x in good])
