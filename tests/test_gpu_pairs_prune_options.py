"""mbavo_pairs_prune_keypoints on the option-laden objects A - D of tests/pairs_oracle.py, held to its numpy restatement
(tests/pairs_prune_ref.py: run_and_check, bit for bit on arrays at full capacity, the device's counts, the host's K, the records and
d_keep), and what comes after a prune held to the pruned set under each pair's own camera.  The prune's own tests build one pinhole
camera, L = 2 and equal K per level; the kernel addresses two slot layouts in one launch -- the filter's state at the offsets of
level = -1, the caller's flag and keep bytes at those of the call's level -- and there a wrong third offset, a level taken for a
slot or the -1 layout used for a level's bytes cannot show.  Here: L = 3 with per-level K and capacities that differ (D), a camera
set (B, D), odd sizes under a packed keyframe (A), a level-0 slice beyond 4096 keypoints (C), clearance-filtered lists (B, D).
What the objects, the keep patterns and min_keep must provide is asserted without a GPU in
tests/test_pairs_prune_hyp_options_inputs.py.

Bounds.  The prune, the evaluation and the LM on compacted copies, and the smoothing: bit for bit.  The evaluation against the
oracle on the rebuilt pruned entries: 1e-9, max |device - oracle| / max |oracle| per array (the packed block and the patch costs of
an entry), the figure of tests/test_gpu_pairs_oracle.py and tests/test_gpu_fullsize.py.  The refinement after the prune: BOUND =
1e-9 with the knife-edge rule of tests/test_gpu_pairs_depth_options.py (pairs_depth_support.knife: from the restatement alone, at
most 1 % of a (pair, level)).  The filter after the prune: pairs_prune_support.FILTER_BOUND, that of tests/test_gpu_pairs_prune.py.
Every figure is printed before it is asserted (-s); the largest per stage and object on an MI355X are in
profiles/r37_prune_hyp_options.txt."""
import contextlib

import numpy as np
import pytest

import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po
import pairs_prune_ref as pref
import pairs_prune_support as psup

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)
BOUND = 1e-9
FILTER = dc.FILTER


@contextlib.contextmanager
def _fresh(ctx, name):
    pb, counts = po.make_object(ctx, name)
    try:
        yield pb, counts
    finally:
        pb.close()


def _between(res, before):
    """0 < kept < K on every served (pair, level) with more than one keypoint."""
    return all(0 < want["K"] < before[key] for key, want in res.items() if before[key] > 1)


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0


def _after_the_prune(orc, mbavo, ctx, pb, name, res, snap):
    """Check 5: evaluation, refinement, smoothing and LM see the pruned set, every pair under its own camera."""
    capi, o = mbavo.capi, po.OBJECTS[name]
    k, n = o["k"], pb.B * pb.L
    E = ctx.lib.mbavo_packed_len(k)
    # the object's own arrays against compacted copies: the same bits
    arr, hold = psup.patched_problems(capi, pb, snap, res)
    assert all(arr[e].K == pb.array[e].K for e in range(n)) and any(arr[e].d_kp_z != pb.array[e].d_kp_z for e in range(n))
    fb_a, pc_a = psup.evaluate(ctx, capi, pb.array, n, k)
    fb_b, pc_b = psup.evaluate(ctx, capi, arr, n, k)
    assert dv.same_bits(fb_a, fb_b) and dv.same_bits(pc_a, pc_b) and np.abs(fb_a).max() > 0
    # against the oracle on every entry as it is now
    off = np.concatenate([[0], np.cumsum([pb.array[e].K for e in range(n)])])
    worst = dict(block=0.0, patch=0.0)
    for e in range(n):
        b, l = e // pb.L, e % pb.L
        p, keep = po.oracle_problem(orc, capi, pb.array[e], k)
        assert p.K == (res[(b, l)]["K"] if (b, l) in res else snap["ents"][(b, l)]["K"]), (name, b, l)
        assert list(pb.array[e].intrinsics) == [v / float(1 << l) for v in po.to_intr(o, b)], (name, b, l)
        ro = orc.evaluate(p)
        d_block = _rel(fb_a[e * E:(e + 1) * E], ro["frame_blocks"][0])
        d_patch = _rel(pc_a[off[e]:off[e + 1]], ro["patch_blocks"][0][:, 0])
        print("%s pair %d level %d K %d after the prune: block %.3g, patch costs %.3g of the oracle's largest (bound %.0e)" % (name, b, l, p.K, d_block, d_patch, BOUND))
        worst = dict(block=max(worst["block"], d_block), patch=max(worst["patch"], d_patch))
    print("FIGURE eval   object %s: block %.3g, patch costs %.3g" % (name, worst["block"], worst["patch"]))
    assert worst["block"] <= BOUND and worst["patch"] <= BOUND, (name, worst)
    if o["cam_of"] is not None:
        counts = np.array([[pb.array[b * pb.L + l].K for l in range(pb.L)] for b in range(pb.B)])
        ds.smooth_check(pb, tag=name + " after the prune", **dc.smooth_opts(name))
        log = []
        ds.refine_check(mbavo, ctx, pb, counts, k, name + " after the prune", BOUND, level=-1, exclude=True, log=log, **dc.REFINE)
        print("FIGURE refine object %s: largest relative difference %.3g, keypoints left out %d of %d"
              % (name, max(x[5] for x in log), sum(x[4] for x in log), sum(x[3] for x in log)))
    # the LM: the same records, fields and knots from the object's arrays and from the copies
    runs = []
    for problems in (pb.array, arr):
        po.set_motion(pb, po.inputs(name)["motion"])
        fields, recs, kinds = dv.run_lm(ctx, capi, pb.B, pb.L, problems, k)
        runs.append((fields, recs, [a.tobytes() for a in pb.knots()]))
    assert runs[0] == runs[1], name
    assert all(len(r) > 0 for r in runs[0][1])  # (the LM did iterate)
    del hold


# ---- 1. every level at once, a subset of pairs; 5. what comes after
@pytest.mark.parametrize("name", NAMES)
def test_every_level_a_subset_of_pairs_and_what_comes_after(orc, mbavo, gpu_ctx, name):
    with _fresh(gpu_ctx, name) as (pb, counts):
        listed = psup.listed_pairs(pb.B)
        keeps = psup.keep_patterns(counts, psup.SEED_ALL)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(psup.SEED_ALL))
        assert np.isin(flags[psup.LEFT_OUT, :counts[psup.LEFT_OUT, 0]], psup.GO).any()  # the pair left out has dropping bytes too
        out, res, snap, stats = pref.run_and_check(pb, listed, level=-1, apply=True, flags=flags, drop_mask=psup.MASK, tag=name + " every level")
        assert sorted(res) == [(b, l) for b in listed for l in range(pb.L)]
        for key, want in res.items():
            assert want["K"] == int(keeps[key].sum()) and np.array_equal(want["keep"].astype(bool), keeps[key]), (name, key)
        assert _between(res, {key: int(counts[key]) for key in res}), name
        assert stats == (1, 1, 4 * pb.B * pb.L + psup.REC * len(listed) * pb.L), (name, stats)
        assert [pb.array[psup.LEFT_OUT * pb.L + l].K for l in range(pb.L)] == counts[psup.LEFT_OUT].tolist()
        print("%s: K before %s, after %s" % (name, counts.tolist(), [[pb.array[b * pb.L + l].K for l in range(pb.L)] for b in range(pb.B)]))
        _after_the_prune(orc, mbavo, gpu_ctx, pb, name, res, snap)


# ---- 2. one level alone, every pair
@pytest.mark.parametrize("name", NAMES)
def test_one_level_alone_every_pair(gpu_ctx, name):
    with _fresh(gpu_ctx, name) as (pb, counts):
        cap = pb.capacities()
        for l in range(pb.L):
            keeps = psup.keep_patterns(counts, psup.SEED_LEVEL + l, levels=[l])
            flags = psup.flag_bytes(pb.B, cap, keeps, np.random.default_rng(psup.SEED_LEVEL + l), level=l)
            assert flags.shape == (pb.B, cap[l])
            out, res, _, stats = pref.run_and_check(pb, None, level=l, apply=True, flags=flags, drop_mask=psup.MASK, tag="%s level %d" % (name, l))
            assert sorted(res) == [(b, l) for b in range(pb.B)]
            assert [r.num_kept for r in out] == [int(keeps[(b, l)].sum()) for b in range(pb.B)], (name, l)
            assert _between(res, {key: int(counts[key]) for key in res}), (name, l)
            assert stats == (1, 1, 4 * pb.B * pb.L + psup.REC * pb.B), (name, l, stats)
        # (the levels above l kept their bits through every call: run_and_check; the last state is every level pruned by its own pattern)
        assert [pb.array[e].K for e in range(pb.B * pb.L)] == [int(psup.keep_patterns(counts, psup.SEED_LEVEL + l, levels=[l])[(b, l)].sum())
                                                               for b in range(pb.B) for l in range(pb.L)]


# ---- 3. with a filter state
@pytest.mark.parametrize("name", ["B", "D"])
def test_with_a_filter_state(mbavo, gpu_ctx, name):
    o = po.OBJECTS[name]
    with _fresh(gpu_ctx, name) as (pb, counts):
        for _ in range(2):
            assert pb.filter_depths(level=-1, apply=True, **FILTER)[0] == 0
        rng = np.random.default_rng(psup.SEED_FILTER)
        psup.random_state(pb, rng)
        listed = psup.listed_pairs(pb.B)
        keeps = psup.keep_patterns(counts, psup.SEED_FILTER)
        out, res, snap, _ = pref.run_and_check(pb, listed, level=-1, apply=True, flags=psup.flags_of(pb, keeps, rng), drop_mask=psup.MASK, use_filter=True,
                                               min_obs=2, rej_limit=4, tag=name + " with a state")
        print(name, "with a state", [pref.record_tuple(r) for r in out])
        assert all(r.by_flag > 0 for r in out if r.num_before > 1) and sum(r.by_filter for r in out) > 0 and _between(res, {key: int(counts[key]) for key in res})
        assert snap["state"] is not None
        # the filter carries on from the moved state: nothing is seeded, and the call equals the restatement fed that state
        none = [[False] * o["L"] for _ in range(o["B"])]
        worst, fil = ds.filter_check(mbavo, gpu_ctx, pb, o["k"], name + " filter after the prune", none, psup.FILTER_BOUND, exclude=True, **FILTER)
        assert all(r.seeded == 0 and r.status == 0 for r in fil)
        assert [r.num_keypoints for r in fil] == [pb.array[e].K for e in range(pb.B * pb.L)]
        print("FIGURE filter object %s: largest relative difference %.3g (bound %.3g)" % (name, worst, psup.FILTER_BOUND))


# ---- 4. min_keep per (pair, level)
def test_min_keep_skips_levels_inside_a_pair(gpu_ctx):
    with _fresh(gpu_ctx, "D") as (pb, counts):
        keeps = psup.keep_patterns(counts, psup.SEED_MIN_KEEP)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(psup.SEED_MIN_KEEP))
        out, res, _, _ = pref.run_and_check(pb, None, level=-1, apply=True, flags=flags, drop_mask=psup.MASK, min_keep=psup.MIN_KEEP_D, tag="D min_keep")
        skipped = np.array([r.skipped for r in out]).reshape(pb.B, pb.L)
        want = np.array([[int(keeps[(b, l)].sum() < psup.MIN_KEEP_D) for l in range(pb.L)] for b in range(pb.B)])
        print("D min_keep %d: survivors %s, skipped %s" % (psup.MIN_KEEP_D, [[int(keeps[(b, l)].sum()) for l in range(pb.L)] for b in range(pb.B)], skipped.tolist()))
        assert np.array_equal(skipped, want) and np.array_equal(skipped, np.array([[res[(b, l)]["record"][6] for l in range(pb.L)] for b in range(pb.B)]))
        assert any(0 < skipped[b].sum() < pb.L for b in range(pb.B))  # served and skipped levels inside one pair
        assert all(pb.array[b * pb.L + l].K == (counts[b, l] if skipped[b, l] else int(keeps[(b, l)].sum())) for b in range(pb.B) for l in range(pb.L))


# ---- 6. a wrong slot must fail
def test_a_wrong_slot_must_fail(gpu_ctx):
    """The comparison sees the fault it is there for: the restatement of level 1 fed level 2's flag bytes -- what a kernel that took
    the wrong slot of the caller's layout would read -- gives other keep bytes than the device, on every pair."""
    import torch
    with _fresh(gpu_ctx, "D") as (pb, counts):
        cap = pb.capacities()
        off = [sum(cap[:l]) for l in range(pb.L)]
        keeps = psup.keep_patterns(counts, psup.SEED_SLOT)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(psup.SEED_SLOT))
        before = pref.snapshot(pb)
        keep = torch.full((pb.B, sum(cap)), 99, dtype=torch.uint8, device="cuda:0")
        rc, out = pb.prune_keypoints(None, level=-1, apply=False, flags=dv.dev(flags)[0], keep=keep, drop_mask=psup.MASK)
        assert rc == 0
        keep = keep.cpu().numpy()
        for b in range(pb.B):
            e = before["ents"][(b, 1)]
            right = pref.prune(e["K"], e["xy"], e["z"], None, flags=flags[b, off[1]:off[1] + cap[1]], apply=0, drop_mask=psup.MASK)
            wrong = pref.prune(e["K"], e["xy"], e["z"], None, flags=flags[b, off[2]:off[2] + cap[1]], apply=0, drop_mask=psup.MASK)
            got = keep[b, off[1]:off[1] + e["K"]]
            assert np.array_equal(got, right["keep"]) and not np.array_equal(got, wrong["keep"]), b
            assert pref.record_tuple(out[b * pb.L + 1]) == right["record"] != wrong["record"], b
