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

import lm_support as lms
import tracking

pytestmark = pytest.mark.gpu


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
    opts = dict(lms.SOLVE, solver_type=solver, fast_solve_ratio=fast)
    host = [tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, opts) for sc in scs]
    pairs = lms.Pairs(mbavo, scs)
    got = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, k, solver, fast))
    kinds = set()
    for b, (g, h) in enumerate(zip(got, host)):
        lms.check_against(g, h["trace"], h["kt"], h["kR"], h["cost"], (k, solver, fast, b))
        lms.check_fields(g, 3)
        kinds |= {r[2] for r in g[1]}
        assert np.abs(g[2][0] - scs[b]["kt0"]).max() > 1e-9  # the knots really moved
    assert 1 in kinds and 2 in kinds


def test_levels_against_oracle(orc, mbavo, gpu_ctx):
    """A few pairs against the oracle's optimizeTrajectory (tracking.run_oracle_tracker), same rules."""
    for k in (4, 2):
        scs = _scenes(orc, k, seeds=[70 + k, 71 + k, 72 + k])
        want = [tracking.run_oracle_tracker(orc, sc, lms.SOLVE) for sc in scs]
        got = lms.run(mbavo, gpu_ctx, lms.Pairs(mbavo, scs), lms.levels_opts(mbavo, k, sync_every=0))
        for b, (g, w) in enumerate(zip(got, want)):
            lms.check_against(g, w["trace"], w["kt"], w["kR"], w["cost"], (k, b))
            lms.check_fields(g, 3)


def test_one_level_is_lm_batch(orc, mbavo, gpu_ctx):
    """L = 1 through the new entry and mbavo_lm_batch on the same one-level problems (each scene's level 0 and, as a second
    batch, its level 1): identical bits -- every record field, the result fields, the knots -- for sync_every 0 and 3."""
    scs = _scenes(orc, 4, seeds=[90, 91, 92, 93])
    for lv in (0, 1):
        pairs = lms.Pairs(mbavo, scs, levels=[lv])
        for se in (0, 3):
            a = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=se), levels=True)
            b = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=se), levels=False)
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
    pairs = lms.Pairs(mbavo, scs)

    def same_bits(got, base, tag):
        assert repr([(x[0], x[1]) for x in got]) == repr([(x[0], x[1]) for x in base]), tag
        for x, y in zip(got, base):
            assert np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1]), tag

    base = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=0))
    same_bits(lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=3)), base, "sync_every")
    got = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=0, groups=2))
    assert [[r[:4] for r in x[1]] for x in got] == [[r[:4] for r in x[1]] for x in base]
    assert sum(x[0][1] for x in base) > 0
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.engine_opts(sample_parallel=-1)
        one = lms.run(mbavo, ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=0))
        for kw in (dict(sync_every=0, groups=2), dict(sync_every=3, groups=2)):
            same_bits(lms.run(mbavo, ctx, pairs, lms.levels_opts(mbavo, 4, **kw)), one, kw)
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
    pool = lms.run(mbavo, gpu_ctx, lms.Pairs(mbavo, pool_sc), lms.levels_opts(mbavo, 4, sync_every=3))
    n = [lms.per_level_iterations(x[1]) for x in pool]
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
    pairs = lms.Pairs(mbavo, [pool_sc[b] for b in pick])
    monkeypatch.setenv("MBAVO_LM_STAMPS", "1")
    capfd.readouterr()
    got = lms.run(mbavo, gpu_ctx, pairs, lms.levels_opts(mbavo, 4, sync_every=0))
    err = capfd.readouterr().err
    monkeypatch.delenv("MBAVO_LM_STAMPS")
    slots = len(re.findall(r"^mbavo lm_batch:\s+slot \d+:", err, re.M))
    nb = [lms.per_level_iterations(x[1]) for x in got]
    bound = max(sum(v + 2 for v in m.values()) for m in nb)
    lock_step = sum(max(m[l] for m in nb) for l in range(3))
    assert bound < lock_step, (nb, bound, lock_step)  # (a precondition of the batch)
    assert 0 < slots <= bound, (slots, bound, lock_step, nb)


def test_levels_argument_errors(orc, mbavo, gpu_ctx):
    """MBAVO_E_ARG (-1) with nothing launched: knot buffers that differ within a pair, L = 0, L = 9, a null problem list, a level
    with another capture-time buffer; the context works afterwards."""
    capi = mbavo.capi
    scs = _scenes(orc, 4, seeds=[150, 151])
    pairs = lms.Pairs(mbavo, scs)
    o = lms.levels_opts(mbavo, 4)
    res = (capi.LmBatchResult * 2)()
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good = lms.run(mbavo, gpu_ctx, pairs, o)
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
    again = lms.run(mbavo, gpu_ctx, pairs, o)
    assert repr([(x[0], x[1]) for x in again]) == repr([(x[0], x[1]) for x in good])
