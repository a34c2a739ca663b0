"""The batched LM (mbavo_lm_batch, mbavo_lm_batch_levels) on dense lists -- one-pixel patches, K in the thousands, what
mbavo_pairs hands it since every semi-dense candidate became a keypoint -- against the host loop (mbavo_optimize_trajectory,
pair after pair) and the oracle, with the rules and the stated tolerances of tests/test_gpu_lm_batch_levels.py: the (level,
iteration, kind, outlier count) sequence exact; costs and model change 1e-5, radius 1e-4, quality 1e-3, knots 1e-4.

k_lm_decide forms the outlier statistics from registers up to K = 512 and in three strided passes over global memory above;
every other test that meets an independent reference has K <= 512.  Here: K on both sides of 512 within one batch and within
one pair (its level switch), K = 511, 512, 513 and 577 in one call under every schedule, and patch costs of exactly 0 (skipped
by the mean and the variance, compared with the bound all the same).  The scenes and the rule their seeds were chosen by (from
the oracle alone, so that no case sits where rounding decides) are in tests/lm_dense.py; tests/test_lm_dense_seeds.py
re-checks them without a GPU.  No case is left out here: a disagreement on a committed seed is a failure."""
import numpy as np
import pytest

import lm_dense as ld
import lm_support as lms
import tracking

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _levels_case(orc, mbavo, gpu_ctx, k, solver, fast):
    """Scenes, the oracle's runs, the host loop's runs and ONE batched run of a (k, solver, fast) case: computed once."""
    def make():
        scs = ld.level_scenes(orc, k, ld.LEVEL_SEEDS[(k, solver)])
        opts = dict(ld.SOLVE, solver_type=solver, fast_solve_ratio=fast)
        want = [tracking.run_oracle_tracker(orc, sc, opts) for sc in scs]
        host = [tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, opts) for sc in scs]
        got = lms.run(mbavo, gpu_ctx, lms.Pairs(mbavo, scs), lms.levels_opts(mbavo, k, solver, fast))
        return scs, want, host, got
    return _cached(("levels", k, solver, fast), make)


def _witness_levels(scs, got):
    K = [[lv["kp_xy"].shape[0] for lv in sc["levels"]] for sc in scs]
    assert all(k0 > 512 for k0, _ in K) and any(k1 <= 512 for _, k1 in K) and any(k1 > 512 for _, k1 in K), K  # both forms in one batch
    assert {sc["F"] for sc in scs} == {1, 2}                                   # the one-frame path and the frame loop
    recs = [g[1] for g in got]
    assert any(ld.flags_large_K(r, k0) for r, (k0, _) in zip(recs, K))         # outliers flagged by the strided passes
    assert any(ld.outliers_change(r) for r in recs)                            # ... and re-counted, not carried along
    assert {1, 2} <= {r[2] for rs in recs for r in rs}
    for g, sc in zip(got, scs):
        assert np.abs(g[2][0] - sc["kt0"]).max() > 1e-9                        # the knots really moved


@pytest.mark.parametrize("k,solver,fast", ld.LEVEL_CASES)
def test_dense_levels_match_host_loop(orc, mbavo, gpu_ctx, k, solver, fast):
    """B = 4 dense pairs (48 x 64: K = 960 | 240; 96 x 128: K = 7488 | 1872; F = 1, 1, 2, 2; two levels, S = 4) in one
    mbavo_lm_batch_levels call against mbavo_optimize_trajectory per pair on the same data and options."""
    scs, _, host, got = _levels_case(orc, mbavo, gpu_ctx, k, solver, fast)
    _witness_levels(scs, got)
    for b, (g, h) in enumerate(zip(got, host)):
        lms.check_against(g, h["trace"], h["kt"], h["kR"], h["cost"], ("host", k, solver, fast, b))
        lms.check_fields(g, 2)


@pytest.mark.parametrize("k,solver,fast", ld.LEVEL_CASES)
def test_dense_levels_against_oracle(orc, mbavo, gpu_ctx, k, solver, fast):
    """The same call against the oracle's optimizeTrajectory (tracking.run_oracle_tracker), same rules."""
    scs, want, _, got = _levels_case(orc, mbavo, gpu_ctx, k, solver, fast)
    _witness_levels(scs, got)
    for b, (g, w) in enumerate(zip(got, want)):
        lms.check_against(g, w["trace"], w["kt"], w["kR"], w["cost"], ("oracle", k, solver, fast, b))
        lms.check_fields(g, 2)


def _one_level_references(orc, mbavo, gpu_ctx, key, scs):
    return _cached(key, lambda: ([tracking.run_oracle_tracker(orc, sc, ld.SOLVE12) for sc in scs],
                                 [tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, ld.SOLVE12) for sc in scs]))


def _check_one_level(got, want, host, tag):
    for b, (g, w, h) in enumerate(zip(got, want, host)):
        lms.check_against(g, h["trace"], h["kt"], h["kR"], h["cost"], ("host",) + tag + (b,))
        lms.check_against(g, w["trace"], w["kt"], w["kR"], w["cost"], ("oracle",) + tag + (b,))
        lms.check_fields(g, 1)
        assert any(r[2] == 1 and r[3] > 0 for r in g[1]), (tag, b)  # an accepted step that flagged outliers


def test_dense_cuts_around_512(orc, mbavo, gpu_ctx):
    """One dense 48 x 64 scene cut to its first K = 511, 512, 513 and 577 keypoints: four problems in one mbavo_lm_batch call
    (F = 1, 12 iterations at most), each against its own host loop and oracle run, under sync_every 0 and 3 with the LM kernels
    summing the tile partials themselves where the list allows (defer_finalize 1) and with the finalize kernels (-1).  The
    schedules give identical records, result fields and knots, bit for bit (retile = -1 as in
    test_lm_batch_deferred_finalize_same_bits: a second tiling would regroup the sums)."""
    scs = ld.cut_scenes(orc, ld.CUT_SEED)
    assert tuple(sc["levels"][0]["kp_xy"].shape[0] for sc in scs) == ld.CUT_K
    want, host = _one_level_references(orc, mbavo, gpu_ctx, "cuts", scs)
    pairs = lms.Pairs(mbavo, scs, levels=[0])
    assert [pairs.array[b].K for b in range(4)] == list(ld.CUT_K) and all(pairs.array[b].P == 1 for b in range(4))
    base = first = None
    for sync_every in (0, 3):
        for defer in (1, -1):
            o = lms.levels_opts(mbavo, 4, sync_every=sync_every, max_it=12)
            o.defer_finalize, o.retile = defer, -1
            got = lms.run(mbavo, gpu_ctx, pairs, o, levels=False)
            _check_one_level(got, want, host, (sync_every, defer))
            bits = (repr([(x[0], x[1]) for x in got]), [(x[2][0].tobytes(), x[2][1].tobytes()) for x in got])
            if base is None:
                base, first = bits, got
            assert bits == base, ("schedules differ", sync_every, defer, [lms.flip_margin(x[1], y[1]) for x, y in zip(got, first)])


@pytest.mark.parametrize("variant", sorted(ld.FLAT_SEEDS))
def test_dense_exact_zero_patch_costs(orc, mbavo, gpu_ctx, variant):
    """A dense pair with a flat rectangle on which keyframe and current image are equal: at least 64 patch costs are exactly
    0.0 at the initial knots and all others above 1e-8 (the oracle's per-patch costs), with K = 512 (statistics from registers)
    and K = 960 (strided passes).  A kernel that counted the zero costs into the mean or the variance would move the bound and
    the outlier count.  On the offset variants (K = 480, 960; lm_dense.flat_scene) the other costs lie so close together that
    the zero costs are beyond the bound: an accepted step counts every one of them as an outlier, which a flagging pass that
    skipped costs below 1e-8 as the first two passes do would not."""
    sc = ld.flat_scene(orc, variant, ld.FLAT_SEEDS[variant])
    K = sc["levels"][0]["kp_xy"].shape[0]
    assert K == {"K512": 512, "K960": 960, "K480_offset": 480, "K960_offset": 960}[variant]
    costs = ld.initial_patch_costs(orc, sc)
    assert int((costs == 0.0).sum()) >= 64 and np.all(costs[costs != 0.0] > 1e-8)
    assert ld.flat_costs_ok(costs, ld.flat_inside(sc))
    want, host = _one_level_references(orc, mbavo, gpu_ctx, ("flat", variant), [sc])
    for sync_every in (0, 3):
        got = lms.run(mbavo, gpu_ctx, lms.Pairs(mbavo, [sc], levels=[0]), lms.levels_opts(mbavo, 4, sync_every=sync_every, max_it=12), levels=False)
        _check_one_level(got, want, host, (variant, sync_every))
        assert ld.flags_the_zero_costs(got[0][1], costs) == variant.endswith("_offset"), (variant, got[0][1])
