"""The committed seeds of tests/lm_dense.py still satisfy the rule they were chosen by (lm_dense.seed_ok: pinned and contracted
oracle agree on the record sequence, every accept and outlier test of the pinned run keeps its margin), and the oracle's runs
on them show what tests/test_gpu_lm_batch_dense.py needs to mean something.  No GPU: a change to the scenes cannot silently
put a case of the GPU file on a decision boundary."""
import pytest

import lm_dense as ld


@pytest.fixture(scope="module")
def fma(orc):
    v = orc.fma_variant()
    if v is None:
        pytest.skip("no FMA build of the oracle on this host")
    return v


@pytest.mark.parametrize("k,solver", sorted(ld.LEVEL_SEEDS))  # (the oracle has no fast_solve_ratio)
def test_level_seeds_keep_the_rule(orc, fma, k, solver):
    opts = dict(ld.SOLVE, solver_type=solver)
    for b, sc in enumerate(ld.level_scenes(orc, k, ld.LEVEL_SEEDS[(k, solver)])):
        ok, why, _ = ld.seed_ok(orc, fma, sc, opts)
        assert ok, (k, solver, b, why)


def test_cut_and_flat_seeds_keep_the_rule(orc, fma):
    for sc in ld.cut_scenes(orc, ld.CUT_SEED) + [ld.flat_scene(orc, v, s) for v, s in ld.FLAT_SEEDS.items()]:
        ok, why, _ = ld.seed_ok(orc, fma, sc, ld.SOLVE12)
        assert ok, (sc["levels"][0]["kp_xy"].shape[0], why)


@pytest.mark.parametrize("k,solver", sorted(ld.LEVEL_SEEDS))
def test_level_scenes_are_not_vacuous(orc, k, solver):
    """K on both sides of 512 in one batch, F = 1 and 2, and in the oracle's run: outliers flagged at K > 512, a count that
    changes between two accepted level-0 steps, accepted and rejected steps."""
    scs = ld.level_scenes(orc, k, ld.LEVEL_SEEDS[(k, solver)])
    K = [[lv["kp_xy"].shape[0] for lv in sc["levels"]] for sc in scs]
    assert all(k0 > 512 for k0, _ in K) and any(k1 <= 512 for _, k1 in K) and any(k1 > 512 for _, k1 in K), K
    assert {sc["F"] for sc in scs} == {1, 2}
    runs = [ld.run_with_margin(orc, sc, dict(ld.SOLVE, solver_type=solver))[0]["trace"] for sc in scs]
    assert any(ld.flags_large_K(tr, k0) for tr, (k0, _) in zip(runs, K))
    assert any(ld.outliers_change(tr) for tr in runs)
    assert {1, 2} <= {r[2] for tr in runs for r in tr}


def test_cut_and_flat_scenes_are_not_vacuous(orc):
    cuts = ld.cut_scenes(orc, ld.CUT_SEED)
    assert tuple(sc["levels"][0]["kp_xy"].shape[0] for sc in cuts) == ld.CUT_K
    flats = {v: ld.flat_scene(orc, v, s) for v, s in ld.FLAT_SEEDS.items()}
    assert {v: sc["levels"][0]["kp_xy"].shape[0] for v, sc in flats.items()} == {"K512": 512, "K960": 960, "K480_offset": 480, "K960_offset": 960}
    for v, sc in flats.items():
        costs = ld.initial_patch_costs(orc, sc)
        assert ld.flat_costs_ok(costs, ld.flat_inside(sc))
        flagged = ld.flags_the_zero_costs(ld.run_with_margin(orc, sc, ld.SOLVE12)[0]["trace"], costs)
        assert flagged == v.endswith("_offset"), v  # the offset variants: an accepted step flags every zero cost
    for sc in cuts + list(flats.values()):
        tr = ld.run_with_margin(orc, sc, ld.SOLVE12)[0]["trace"]
        assert any(r[2] == 1 and r[3] > 0 for r in tr), tr  # (an accepted step that flagged outliers: the statistics ran and mattered)
