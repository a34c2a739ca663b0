"""Coarse-to-fine alignment of a batch of keyframe pairs (640 x 480, L pyramid levels, k = 4, S = 8 on every level), three ways,
from the same initial knots, best of `reps` repetitions each ending in a device synchronisation:
  (a) mbavo_lm_batch_levels: every pair's whole pyramid in ONE device-side call (a pair goes on to its next level when its
      current one ends);
  (b) L chained mbavo_lm_batch calls, coarse to fine (every level a call; the pairs move through the levels in lock-step);
  (c) mbavo_optimize_trajectory pair after pair (the host-driven loop), only for B <= host_max.
The reference's loop options (max 50 iterations per level, early exit at an absolute cost decrease below 1e-3).  Also reports the
LM slots per call (the per-slot lines MBAVO_LM_STAMPS=1 prints, one untimed run each; batches of 384+ pairs run as two groups,
each printing its own) and checks that (a) and (b) agree on every
pair's discrete records (level, iteration, kind, outliers).
Usage: python tools/lm_levels_bench.py [B ...]  (default 64 512)      one text block per B, then one JSON line per B"""
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

L_LEVELS, K_DEG, MAX_IT, CAP = 4, 4, 50, 256


def _opts(capi, sync_every=0):
    o = capi.LmBatchOpts()
    o.spline_deg_k, o.max_num_iterations, o.max_consecutive_nonmonotonic_steps = K_DEG, MAX_IT, 5
    o.solver_type, o.sync_every = 0, sync_every
    o.min_step_quality, o.min_abs_cost_decrease, o.max_chi_square_error = 0.5, 1e-3, 3.0
    return o


def _stderr_of(fn):
    """fn()'s output on file descriptor 2 (the library prints its stamps there)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace")


def _slots(text):
    return len(re.findall(r"^mbavo lm_batch:\s+slot \d+:", text, re.M))


def run_levels(M, ctx, pp, trace=True):
    """(a): one call; per pair the records [(level, iter, kind, outliers)] (trace=True) and the results."""
    capi = M.capi
    B, L = pp.B, pp.L
    res = (capi.LmBatchResult * B)()
    tr = (capi.TraceRec * (B * CAP))() if trace else None
    rc = ctx.lib.mbavo_lm_batch_levels(ctx.handle, B, L, pp.array, C.byref(_opts(capi)), res, tr, CAP if trace else 0)
    assert rc == 0, rc
    recs = [[(t.level, t.iter, t.kind, t.num_outliers) for t in tr[b * CAP:b * CAP + res[b].num_trace]] for b in range(B)] if trace else None
    return recs, res


def level_arrays(M, pp):
    """(b)'s inputs: for each level l one B-entry mbavo_problem array (the entries b*L + l of the pyramid list)."""
    capi = M.capi
    out = []
    for l in range(pp.L):
        a = (capi.Problem * pp.B)()
        for b in range(pp.B):
            C.memmove(C.byref(a[b]), C.byref(pp.array[b * pp.L + l]), C.sizeof(capi.Problem))
        out.append(a)
    return out


def run_chained(M, ctx, pp, arrays, trace=True):
    """(b): L mbavo_lm_batch calls, coarsest level first; records as (a) writes them (the level put in)."""
    capi = M.capi
    B, L = pp.B, pp.L
    o = _opts(capi)
    res = (capi.LmBatchResult * B)()
    tr = (capi.TraceRec * (B * CAP))() if trace else None
    recs = [[] for _ in range(B)]
    for l in range(L - 1, -1, -1):
        rc = ctx.lib.mbavo_lm_batch(ctx.handle, B, arrays[l], C.byref(o), res, tr, CAP if trace else 0)
        assert rc == 0, rc
        if trace:
            for b in range(B):
                recs[b] += [(l, t.iter, t.kind, t.num_outliers) for t in tr[b * CAP:b * CAP + res[b].num_trace]]
    return recs


def run_host(M, ctx, pp, b):
    """(c) for one pair: mbavo_optimize_trajectory over its L levels; its records."""
    capi = M.capi
    lv, intr, cap, exp, t0, dt, kt, kR, huber = pp.levels_of(b)
    to = capi.TrackOpts()
    to.num_levels, to.spline_deg_k, to.max_num_iterations, to.max_consecutive_nonmonotonic_steps, to.solver_type = pp.L, K_DEG, MAX_IT, 5, 0
    for i in range(4):
        to.intrinsics[i] = float(intr[i])
    to.huber_k, to.min_step_quality, to.min_abs_cost_decrease, to.max_chi_square_error = huber, 0.5, 1e-3, 3.0
    start, cost = np.zeros(1, np.int32), np.zeros(1)
    tr = (capi.TraceRec * CAP)()
    n = ctx.lib.mbavo_optimize_trajectory(ctx.handle, C.byref(to), lv, 1, capi.dp(cap), capi.dp(exp), t0, dt, capi.dp(kt), capi.dp(kR),
                                          4, capi.ip(start), capi.dp(cost), tr, CAP)
    assert n > 0, n
    return [(t.level, t.iter, t.kind, t.num_outliers) for t in tr[:n]]


def best_ms(fn, reset, reps):
    import torch
    times = []
    for _ in range(reps):
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return 1e3 * min(times)


def bench(M, ctx, B, reps=5, host_max=64, seed=1):
    from mba_vo_amd import workloads
    pp = workloads.RenderedPairPyramids(ctx, B, L=L_LEVELS, S=8, k=K_DEG, seed=seed)
    arrays = level_arrays(M, pp)
    out = {"B": B, "groups": 2 if B >= 384 else 1, "L": pp.L, "H": pp.H, "W": pp.W, "k": K_DEG, "S": 8, "max_iterations_per_level": MAX_IT, "reps": reps,
           "K_per_level_mean": [round(float(np.mean([pp.array[b * pp.L + l].K for b in range(B)])), 1) for l in range(pp.L)]}
    # records (untimed): (a) against (b)
    pp.reset_knots()
    ra, res = run_levels(M, ctx, pp)
    pp.reset_knots()
    rb = run_chained(M, ctx, pp, arrays)
    out["records_a_eq_b"] = ra == rb
    out["pairs_records_differ"] = sum(x != y for x, y in zip(ra, rb))
    n = [{l: max(r[1] for r in rec if r[0] == l) for l in range(pp.L)} for rec in ra]
    out["iterations_total"] = int(sum(res[b].iterations for b in range(B)))
    out["iterations_per_level_max"] = [max(m[l] for m in n) for l in range(pp.L)]
    out["slots_bound_own_pace"] = max(sum(m[l] + 1 for l in range(pp.L)) for m in n)   # max_b sum_l (n_bl + 1)
    out["slots_bound_lock_step"] = sum(max(m[l] for m in n) + 1 for l in range(pp.L))  # sum_l max_b (n_bl + 1)
    # slots per call, counted (one untimed run each, MBAVO_LM_STAMPS=1 prints one line per slot)
    os.environ["MBAVO_LM_STAMPS"] = "1"
    try:
        pp.reset_knots()
        out["slots_a"] = _slots(_stderr_of(lambda: run_levels(M, ctx, pp, trace=False)))
        pp.reset_knots()
        out["slots_b"] = _slots(_stderr_of(lambda: run_chained(M, ctx, pp, arrays, trace=False)))
    finally:
        del os.environ["MBAVO_LM_STAMPS"]
    # timings (no trace: the form a user of the batch calls)
    for _ in range(2):  # warm: arenas sized, layouts built
        pp.reset_knots()
        run_levels(M, ctx, pp, trace=False)
        pp.reset_knots()
        run_chained(M, ctx, pp, arrays, trace=False)
    ta = best_ms(lambda: run_levels(M, ctx, pp, trace=False), pp.reset_knots, reps)
    tb = best_ms(lambda: run_chained(M, ctx, pp, arrays, trace=False), pp.reset_knots, reps)
    out["a_levels_one_call_ms"] = round(ta, 3)
    out["b_chained_lm_batch_ms"] = round(tb, 3)
    out["b_over_a"] = round(tb / ta, 3)
    if B <= host_max:
        def host_all():
            for b in range(B):
                run_host(M, ctx, pp, b)
        run_host(M, ctx, pp, 0)
        tc = best_ms(host_all, pp.reset_knots, max(1, reps // 2))
        out["c_host_loop_pair_after_pair_ms"] = round(tc, 3)
        out["c_over_a"] = round(tc / ta, 2)
        out["records_a_eq_c"] = sum(run_host(M, ctx, pp, b) == ra[b] for b in range(B)) == B
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    Bs = [int(a) for a in sys.argv[1:]] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lines = []
    for B in Bs:
        r = bench(mbavo, ctx, B)
        lines.append(r)
        print("B = %d pairs, %d levels of %dx%d (K per level %s), k = %d:" % (B, r["L"], r["W"], r["H"], r["K_per_level_mean"], r["k"]))
        g = " (lines of %d groups)" % r["groups"] if r["groups"] > 1 else ""
        print("  (a) mbavo_lm_batch_levels, one call      %9.3f ms   %d slots%s" % (r["a_levels_one_call_ms"], r["slots_a"], g))
        print("  (b) %d chained mbavo_lm_batch calls       %9.3f ms   %d slots%s   (b / a = %.3f)" % (r["L"], r["b_chained_lm_batch_ms"], r["slots_b"], g, r["b_over_a"]))
        if "c_host_loop_pair_after_pair_ms" in r:
            print("  (c) mbavo_optimize_trajectory x %d pairs %9.3f ms            (c / a = %.2f)" % (B, r["c_host_loop_pair_after_pair_ms"], r["c_over_a"]))
        print("  iterations: %d in all, per level at most %s; slot bounds: own pace %d, lock-step %d" % (
            r["iterations_total"], r["iterations_per_level_max"], r["slots_bound_own_pace"], r["slots_bound_lock_step"]))
        print("  discrete records (a) == (b): %s (%d pairs differ)%s" % (r["records_a_eq_b"], r["pairs_records_differ"],
              "; (a) == (c): %s" % r["records_a_eq_c"] if "records_a_eq_c" in r else ""))
        sys.stdout.flush()
    for r in lines:
        print(json.dumps(r))
