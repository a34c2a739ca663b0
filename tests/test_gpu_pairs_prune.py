"""mbavo_pairs_prune_keypoints on an MI355X against its numpy restatement (tests/pairs_prune_ref.py), bit for bit: the keypoint
arrays and the filter's state at their full capacity (so the entries from the new count on too), the device's counts, K of
mbavo_pairs_problems, the records, d_keep; pairs not listed keep their bytes.

Objects come from prepare_points on the 64 x 48 scene of tests/pairs_refine_scene.py (B = 3, L = 2, every_candidate = 1 for the
capacity, border 0), so K is the test's to choose.  A point list may not be longer than the smallest level's capacity, 768 here, so
K = 1025 alone runs on 96 x 64 images (level 1 holds 1536), still B = 3 and L = 2.  The pairs listed are 0 and 2; pair 1 gets drop
flags as well and must stay as it is.

The filter's tolerance in test_filter_carries_on_from_the_moved_state is that of tests/test_gpu_pairs_filter.py, min(8 x 3.23e-14,
1e-9), 3.23e-14 being the largest relative difference measured there on an MI355X (profiles/r31_pairs_filter.txt)."""
import ctypes as C

import numpy as np
import pytest

import pairs_cases
import pairs_depth_support as ds
import pairs_device as dv
import pairs_prune_ref as pref
import pairs_prune_support as psup
import pairs_refine_scene as sc

pytestmark = pytest.mark.gpu

E_ARG = -1
B, L, H, W = 3, 2, sc.H, sc.W
LISTED = [0, 2]
KS = (0, 1, 63, 64, 65, 255, 256, 257, 600, 1025)
PATTERNS = ("all", "none", "first", "last", "alternating", "seam", "random")
MASK, FILTER_BOUND, REC = psup.MASK, psup.FILTER_BOUND, psup.REC
_flags_of, _random_state, _patched_problems, _evaluate = psup.flags_of, psup.random_state, psup.patched_problems, psup.evaluate


def _object(ctx, nb=B, h=H, w=W, sel=slice(None)):
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, nb, L=L, H=h, W=w, S=sc.S, k=sc.K_DEG, N=sc.N, cell=0, thresh=-1.0, border=0, every_candidate=True, huber=sc.HUBER,
                             intr=sc.INTR)
    m = sc.motion()
    assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    return pb


def _images(h=H, w=W):
    if (h, w) == (H, W):
        c = sc.scene()
        return dv.dev(np.ascontiguousarray(c["sharp"]), np.ascontiguousarray(c["blur"]))
    sharp, _, blur = pairs_cases.inputs(B, h, w, seed=4, special=False)
    return dv.dev(sharp, blur)


def _points(K, seed, h=H, w=W, inside=0):
    """B lists of K level-0 points that every level keeps (x <= w - 2, y <= h - 2: level 1's pixel is inside), at the scene's depths."""
    rng = np.random.default_rng(seed)
    depth = sc.scene()["depth"]
    out = []
    for b in range(B):
        xy = np.stack([rng.integers(inside, w - 1 - inside, K), rng.integers(inside, h - 1 - inside, K)], 1).astype(np.float64)
        z = depth[b][xy[:, 1].astype(int) % H, xy[:, 0].astype(int) % W].astype(np.float64) if K else np.zeros(0)
        out.append((xy, z))
    return out


def _keep_pattern(name, K, rng):
    keep = np.ones(K, bool)
    if name == "none":
        keep[:] = False
    elif name == "first":
        keep[1:] = False
    elif name == "last":
        keep[:-1] = False
    elif name == "alternating":
        keep[1::2] = False
    elif name == "seam":  # a dropped run across the last tile seam (256 i) inside the slice, else the wave seam, else the middle
        s = 256 * ((K - 1) // 256) if K > 256 else (64 if K > 64 else K // 2)
        keep[max(s - 20, 0):s + 20] = False
    elif name == "random":
        keep = rng.uniform(size=K) < 0.7
    return keep


def _poke_tails(pb, rng):
    """Random bits behind every (pair, level)'s keypoints, so that an entry written from the new count on shows."""
    cap = pb.capacities()
    for e in range(pb.B * pb.L):
        q, c = pb.array[e], cap[e % pb.L]
        if c > q.K:
            dv.poke(q.d_kp_xy + 16 * q.K, rng.uniform(-9, 9, 2 * (c - q.K)))
            dv.poke(q.d_kp_z + 8 * q.K, rng.uniform(-9, 9, c - q.K))


@pytest.mark.parametrize("K", KS)
def test_K_and_keep_patterns(gpu_ctx, K):
    h, w = (H, W) if K <= 768 else (64, 96)
    pb = _object(gpu_ctx, h=h, w=w)
    try:
        sharp, blur = _images(h, w)
        pts = _points(K, 100 + K, h, w)
        rng = np.random.default_rng(K)
        # "alternating" once before the filter's first call (no state to move), then every pattern with a state
        for it, name in enumerate(("alternating",) + PATTERNS):
            counts = pb.prepare_points(sharp, blur, pts)
            assert (counts == K).all(), counts
            _poke_tails(pb, rng)
            if it == 1:
                assert pb.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0
            if it >= 1:
                _random_state(pb, rng)
            keeps = {(b, l): _keep_pattern(name, K, rng) for b in range(B) for l in range(L)}
            flags = _flags_of(pb, keeps, rng)
            tag = "K %d %s%s" % (K, name, "" if it else " (no state)")
            out, res, _, stats = pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=flags, drop_mask=MASK, tag=tag)
            for (b, l), want in res.items():
                assert want["K"] == int(keeps[(b, l)].sum()) and np.array_equal(want["keep"].astype(bool), keeps[(b, l)]), (tag, b, l)
            assert stats == (1, 1, 4 * B * L + REC * len(LISTED) * L), (tag, stats)
            assert (pb.prune_stats()[0], pb.prune_stats()[1]) == (1, 1)  # (the count-only call of the check: with records, one wait)
    finally:
        pb.close()


@pytest.fixture(scope="module")
def dense(gpu_ctx):
    """The every-candidate object of the scene: 3072 keypoints at level 0 (12 tiles), 768 at level 1, the filter called twice."""
    pb = _object(gpu_ctx)
    c = sc.scene()
    sharp, blur = _images()
    depth = dv.dev(np.ascontiguousarray(c["depth"]))[0]
    counts = pb.prepare(sharp, depth, blur)
    assert counts.tolist() == [[H * W, H * W // 4]] * B, counts
    yield dict(pb=pb, sharp=sharp, blur=blur, depth=depth)
    pb.close()


def test_every_candidate_object(gpu_ctx, dense):
    pb = dense["pb"]
    rng = np.random.default_rng(5)
    pb.prepare(dense["sharp"], dense["depth"], dense["blur"])
    assert pb.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0
    _random_state(pb, rng)
    keeps = {(b, l): _keep_pattern("random", pb.array[b * L + l].K, rng) for b in range(B) for l in range(L)}
    out, res, _, stats = pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=_flags_of(pb, keeps, rng), drop_mask=MASK, tag="every candidate")
    assert all(0 < res[(b, l)]["K"] < len(keeps[(b, l)]) for b in LISTED for l in range(L))
    assert stats == (1, 1, 4 * B * L + REC * len(LISTED) * L)
    # one level alone, every pair (n = 0, no list): the other level keeps its bytes (run_and_check), the layout is that level's
    pb.prepare(dense["sharp"], dense["depth"], dense["blur"])
    cap = pb.capacities()
    fl1 = np.where(rng.uniform(size=(B, cap[1])) < 0.5, 3, 40).astype(np.uint8)
    out, res, _, stats = pref.run_and_check(pb, None, level=1, apply=True, flags=fl1, drop_mask=MASK, tag="level 1")
    assert [r.num_kept for r in out] == [int((fl1[b] == 40).sum()) for b in range(B)] and stats == (1, 1, 4 * B * L + REC * B)


def _prepared_small(ctx, K=300, seed=7, sel=slice(None), nb=B, inside=8):
    pb = _object(ctx, nb=nb, sel=sel)
    sharp, blur = _images()
    pts = _points(K, seed, inside=inside)[sel]
    counts = pb.prepare_points(sharp[sel].contiguous(), blur[sel].contiguous(), pts)
    assert (counts == K).all()
    return pb, sharp, blur, pts


def test_apply_0_changes_nothing_and_reports_what_apply_1_does(gpu_ctx):
    pb, sharp, blur, pts = _prepared_small(gpu_ctx)
    solo, _, _, _ = _prepared_small(gpu_ctx, sel=slice(2, 3), nb=1)
    try:
        rng = np.random.default_rng(3)
        for o in (pb, solo):
            assert o.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0 and o.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0
        keeps = {(b, l): _keep_pattern("random", 300, rng) for b in range(B) for l in range(L)}
        flags = _flags_of(pb, keeps, rng)
        crit = dict(drop_mask=MASK, use_filter=True, min_obs=1, check_depth=True, z_min=0.5, z_max=3.5)
        held = pref.snapshot(pb)
        dry, res0, after, stats = pref.run_and_check(pb, LISTED, apply=False, flags=flags, min_keep=10, tag="apply 0", **crit)
        assert pref.unchanged(pb, held, after) and stats == (1, 1, REC * len(LISTED) * L)
        again, _, after, _ = pref.run_and_check(pb, LISTED, apply=False, flags=flags, min_keep=10, tag="apply 0 again", **crit)
        assert bytes(again) == bytes(dry) and pref.unchanged(pb, held, after)
        # without records a count-only call waits for nothing and still changes nothing
        rc, none = pb.prune_keypoints(LISTED, apply=False, flags=dv.dev(flags)[0], want_records=False, min_keep=10, **crit)
        assert rc == 0 and none is None and pb.prune_stats() == (1, 0, 0) and pref.unchanged(pb, held, pref.snapshot(pb))
        # pair 2 alone in a one-pair object: the same record and, applied, the same bits as inside the batch
        cap = pb.capacities()
        f_solo = np.ascontiguousarray(flags[2:3])
        rs, res_solo, snap_solo, _ = pref.run_and_check(solo, None, apply=True, flags=f_solo, min_keep=10, tag="one pair", **crit)
        wet, res1, snap, stats = pref.run_and_check(pb, LISTED, apply=True, flags=flags, min_keep=10, tag="apply 1", **crit)
        assert bytes(wet) == bytes(dry) and stats == (1, 1, 4 * B * L + REC * len(LISTED) * L)
        assert any(r.by_flag for r in wet) and any(r.num_kept < r.num_before for r in wet)
        assert bytes(rs) == bytes(wet)[REC * L:]
        for l in range(L):
            a, s = snap["ents"][(2, l)], snap_solo["ents"][(0, l)]
            assert a["K"] == s["K"] and dv.same_bits(a["xy"][:a["K"]], s["xy"][:s["K"]]) and dv.same_bits(a["z"][:a["K"]], s["z"][:s["K"]]), l
            for key in snap["state"]:
                o = sum(cap[:l])
                assert np.array_equal(snap["state"][key][2, o:o + a["K"]], snap_solo["state"][key][0, o:o + a["K"]]), (l, key)
    finally:
        pb.close(); solo.close()


def test_min_keep_holds_back_a_level_one_survivor_short(gpu_ctx):
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=300)
    try:
        rng = np.random.default_rng(8)
        keeps = {(b, l): np.ones(300, bool) for b in range(B) for l in range(L)}
        for b, l, n in ((0, 0, 99), (0, 1, 100), (2, 0, 101), (2, 1, 0)):  # survivors, against min_keep = 100
            keeps[(b, l)][:] = False
            keeps[(b, l)][rng.permutation(300)[:n]] = True
        out, res, _, _ = pref.run_and_check(pb, LISTED, apply=True, flags=_flags_of(pb, keeps, rng), drop_mask=MASK, min_keep=100, tag="min_keep")
        got = [(r.num_before, r.num_kept, r.by_flag, r.skipped) for r in out]
        assert got == [(300, 300, 201, 1), (300, 100, 200, 0), (300, 101, 199, 0), (300, 300, 300, 1)], got
        assert [pb.array[e].K for e in (0, 1, 4, 5)] == [300, 100, 101, 300]
    finally:
        pb.close()


def test_each_criterion_alone_and_all_together(gpu_ctx):
    """Flags of a real smoothing on planted wrong depths, of a real report on level 0, the filter's criteria after two filter calls,
    the depth check with NaN, 0 and the limits themselves."""
    import torch
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=400, inside=8)
    try:
        rng = np.random.default_rng(12)
        cap = pb.capacities()

        def fresh():
            pb.prepare_points(sharp, blur, pts)
            for e in range(B * L):  # one keypoint in eight at a wrong depth; a NaN, a zero and the limits themselves at every level's start
                q = pb.array[e]
                z = dv.peek(q.d_kp_z, q.K, np.float64)
                z[np.arange(q.K) % 8 == 5] *= 1.6
                z[:4] = [np.nan, 0.0, 1.5, 2.5]
                dv.poke(q.d_kp_z, z)
            for _ in range(2):
                assert pb.filter_depths(level=-1, prior_rel_sigma=0.1, gate_chi2=4.0)[0] == 0

        # the smoothing's class bytes (0 invalid, 3 outlier), level = -1
        fresh()
        sm = torch.full((B, sum(cap)), 77, dtype=torch.uint8, device="cuda:0")
        assert pb.smooth_depths(3, min_support=2, max_rel_diff=0.1, fill=False, level=-1, flags=sm)[0] == 0
        sm = sm.cpu().numpy()
        out, res, _, _ = pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=sm, drop_mask=(1 << 0) | (1 << 3), tag="smooth flags")
        print("smooth flags", [pref.record_tuple(r) for r in out])
        assert all(r.by_flag >= 2 and r.num_kept > 0 and r.by_depth == r.by_filter == 0 for r in out)
        assert all(res[(b, l)]["keep"][:2].tolist() == [0, 0] for b in LISTED for l in range(L))  # the NaN and the zero: the smoothing's class 0
        assert all(3 in sm[b, :400] for b in LISTED)  # outliers among the planted depths of level 0
        # the report's chi flags, level 0 (B x cap0 as the report writes them)
        fresh()
        chi = torch.full((B, cap[0]), 9, dtype=torch.uint8, device="cuda:0")
        pb.report(1.5, flags=chi)
        chi = chi.cpu().numpy()
        out, res, _, _ = pref.run_and_check(pb, LISTED, level=0, apply=True, flags=chi, drop_mask=1 << 1, tag="chi flags")
        assert [r.by_flag for r in out] == [int((chi[b, :400] == 1).sum()) for b in LISTED] and all(0 < r.by_flag < 400 for r in out)
        # the filter's criteria
        fresh()
        st, off = ds.filter_state(pb)
        for tag, kw in (("min_info", dict(min_info=float(np.nanmedian(st["info"][0, :400])))), ("min_obs", dict(min_obs=2)), ("rej_limit", dict(rej_limit=1))):
            if tag != "min_info":
                fresh()
            out, res, _, _ = pref.run_and_check(pb, LISTED, level=-1, apply=True, use_filter=True, tag=tag, **kw)
            print(tag, [pref.record_tuple(r) for r in out])
            # (n_obs = 0 on the NaN and the zero of every level; whether the gate rejected anything is the filter's to say: the
            # restatement on the real state is the check there)
            assert all(r.by_flag == r.by_depth == 0 for r in out) and (tag == "rej_limit" or all(r.by_filter > 0 for r in out)), tag
        # the depth check: NaN and 0 go, the limits themselves stay
        fresh()
        out, res, _, _ = pref.run_and_check(pb, LISTED, level=-1, apply=True, check_depth=True, z_min=1.5, z_max=2.5, tag="depth")
        assert res[(0, 0)]["keep"][:4].tolist() == [0, 0, 1, 1] and all(r.by_depth > 0 and r.by_flag == r.by_filter == 0 for r in out)
        # all together: every verdict under the first criterion that holds
        fresh()
        sm = torch.full((B, sum(cap)), 77, dtype=torch.uint8, device="cuda:0")
        assert pb.smooth_depths(3, min_support=2, max_rel_diff=0.1, fill=False, level=-1, flags=sm)[0] == 0
        out, res, _, _ = pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=sm.cpu().numpy(), drop_mask=(1 << 0) | (1 << 3), check_depth=True, z_min=1.5,
                                            z_max=2.5, use_filter=True, min_obs=2, rej_limit=2, min_keep=5, tag="all together")
        print("all together", [pref.record_tuple(r) for r in out])
        assert all(r.by_flag >= 2 for r in out) and sum(r.by_depth for r in out) > 0
    finally:
        pb.close()


def test_filter_carries_on_from_the_moved_state(gpu_ctx, mbavo):
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=300, inside=8)
    try:
        k = sc.K_DEG
        opts = dict(prior_rel_sigma=0.1, sigma_i=2.0, gate_chi2=9.0)
        ALL, NONE = [[True] * L] * B, [[False] * L] * B
        ds.filter_check(mbavo, gpu_ctx, pb, k, "filter 1", ALL, FILTER_BOUND, first=True, **opts)
        ds.filter_check(mbavo, gpu_ctx, pb, k, "filter 2", NONE, FILTER_BOUND, **opts)
        rng = np.random.default_rng(2)
        keeps = {(b, l): _keep_pattern("random", 300, rng) for b in range(B) for l in range(L)}
        # (run_and_check reads the state through mbavo_pairs_filter_state before and after: the compacted state is what it shows)
        pref.run_and_check(pb, LISTED, level=0, apply=True, flags=_flags_of(pb, keeps, rng)[:, :pb.capacities()[0]].copy(), drop_mask=MASK, tag="prune")
        assert [pb.array[e].K for e in range(B * L)] == [int(keeps[(0, 0)].sum()), 300, 300, 300, int(keeps[(2, 0)].sum()), 300]
        # the third call seeds nothing -- not the pruned level, not the pair's other level -- and equals the restatement fed the moved state
        worst, out = ds.filter_check(mbavo, gpu_ctx, pb, k, "filter 3", NONE, FILTER_BOUND, **opts)
        assert all(r.seeded == 0 and r.status == 0 for r in out) and out[0].num_keypoints == int(keeps[(0, 0)].sum())
        print("filter after the prune: largest relative difference %.3g (bound %.3g)" % (worst, FILTER_BOUND))
        # a level that was stale before stays stale: new keypoints for pair 0, a prune, and the filter seeds pair 0 alone
        pb.update_points(None, [0], sharp[:1].contiguous(), pts[:1])
        out, _, _, _ = pref.run_and_check(pb, [0], level=-1, apply=True, check_depth=True, z_min=float(np.median(pts[0][1])), tag="prune a stale pair")
        assert all(0 < r.num_kept < r.num_before for r in out)
        seeded = [[b == 0] * L for b in range(B)]
        ds.filter_check(mbavo, gpu_ctx, pb, k, "filter 4", seeded, FILTER_BOUND, **opts)
    finally:
        pb.close()


def test_the_smoothing_rebuilds_its_index_after_a_prune(gpu_ctx):
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=600)
    try:
        rng = np.random.default_rng(4)
        opts = dict(radius=3, min_support=2, max_rel_diff=0.1, strength=0.7, fill=1)
        ds.smooth_check(pb, tag="before", **opts)
        assert pb.smooth_stats()[0] == 2  # index and gather
        ds.smooth_check(pb, tag="standing index", **opts)
        assert pb.smooth_stats()[0] == 1
        keeps = {(b, l): _keep_pattern("random", 600, rng) for b in range(B) for l in range(L)}
        pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=_flags_of(pb, keeps, rng), drop_mask=MASK, tag="prune")
        # brute force on the compacted keypoints, bit for bit, no rebuild asked for: a stale index would hold the old places
        ds.smooth_check(pb, tag="after the prune", **opts)
        assert pb.smooth_stats()[0] == 2
        # a prune that drops nothing leaves the index standing
        pref.run_and_check(pb, LISTED, level=-1, apply=True, tag="nothing to drop")
        ds.smooth_check(pb, tag="after an empty prune", **opts)
        assert pb.smooth_stats()[0] == 1
    finally:
        pb.close()


def test_lm_on_the_pruned_object_equals_lm_on_compacted_copies(gpu_ctx, mbavo):
    capi = mbavo.capi
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=500, inside=8)
    try:
        rng = np.random.default_rng(6)
        k = sc.K_DEG
        keeps = {(b, l): _keep_pattern("random", 500, rng) for b in range(B) for l in range(L)}
        out, res, snap, _ = pref.run_and_check(pb, LISTED, level=-1, apply=True, flags=_flags_of(pb, keeps, rng), drop_mask=MASK, tag="prune")
        arr, hold = _patched_problems(capi, pb, snap, res)
        assert all(arr[e].K == pb.array[e].K for e in range(B * L)) and arr[0].d_kp_z != pb.array[0].d_kp_z and arr[0].K < 500
        fb_a, pc_a = _evaluate(gpu_ctx, capi, pb.array, B * L, k)
        fb_b, pc_b = _evaluate(gpu_ctx, capi, arr, B * L, k)
        assert dv.same_bits(fb_a, fb_b) and dv.same_bits(pc_a, pc_b) and np.abs(fb_a).max() > 0
        m = sc.motion()
        runs = []
        for problems in (pb.array, arr):
            assert pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]) == 0
            fields, recs, kinds = dv.run_lm(gpu_ctx, capi, B, L, problems, k)
            runs.append((fields, recs, [a.tobytes() for a in pb.knots()]))
        assert runs[0] == runs[1]
        assert all(len(r) > 0 for r in runs[0][1])  # (the LM did iterate)
    finally:
        pb.close()


def test_rejections_leave_the_object_as_it_is(gpu_ctx, mbavo):
    import torch
    lib, capi = gpu_ctx.lib, mbavo.capi
    fresh = _object(gpu_ctx, nb=1, sel=slice(0, 1))
    assert fresh.prune_keypoints(apply=True)[0] == E_ARG and fresh.prune_stats() == (0, 0, 0)  # before the first prepare
    fresh.close()
    pb, sharp, blur, pts = _prepared_small(gpu_ctx, K=100)
    try:
        cap = pb.capacities()
        flags = torch.full((B, sum(cap)), 3, dtype=torch.uint8, device="cuda:0")
        held = pref.snapshot(pb)
        nan, inf = float("nan"), float("inf")
        bad = [dict(level=-2), dict(level=L), dict(apply=2), dict(apply=-1), dict(use_filter=2), dict(check_depth=-1), dict(min_obs=-1), dict(rej_limit=-1),
               dict(min_keep=-1), dict(min_info=-1.0), dict(min_info=nan), dict(min_info=inf), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=-1.0),
               dict(z_max=inf), dict(z_min=3.0, z_max=2.0), dict(z_min=3.0, z_max=2.0, check_depth=1),
               dict(use_filter=1, min_obs=1)]  # (use_filter = 1: no filter call yet -- what the smoothing answers to weights = 1)
        for kw in bad:
            o = pref.opts_struct(capi, **dict(dict(apply=1, drop_mask=1 << 3), **kw))
            assert pref.call(lib, pb.handle, LISTED, o, flags=flags.data_ptr()) == E_ARG, kw
            assert pb.prune_stats() == (0, 0, 0), kw
        assert pb.smooth_depths(2, weights=1)[0] == E_ARG  # (the same answer)
        o = pref.opts_struct(capi, apply=1, drop_mask=1 << 3)
        assert pref.call(lib, pb.handle, LISTED, o, flags=None) == E_ARG  # drop_mask without flags
        assert pref.call(lib, pb.handle, LISTED, None, flags=flags.data_ptr()) == E_ARG
        o.reserved[2] = 1
        assert pref.call(lib, pb.handle, LISTED, o, flags=flags.data_ptr()) == E_ARG
        o.reserved[2] = 0
        for lst in ([0, 0], [2, 0], [-1], [B], [0, 1, 2, 2]):  # duplicate, descending, out of range, too long
            assert pref.call(lib, pb.handle, lst, o, flags=flags.data_ptr()) == E_ARG, lst
        keys = np.array([0], np.int32)
        assert lib.mbavo_pairs_prune_keypoints(pb.handle, 1, None, C.byref(o), flags.data_ptr(), None, None) == E_ARG  # n without a list
        assert lib.mbavo_pairs_prune_keypoints(pb.handle, 0, keys.ctypes.data_as(C.POINTER(C.c_int)), C.byref(o), flags.data_ptr(), None, None) == E_ARG
        assert pb.prune_stats() == (0, 0, 0)
        assert pref.unchanged(pb, held, pref.snapshot(pb)) and (pref.device_counts(pb) == 100).all()
        # the same options, accepted: every listed keypoint goes (flag 3), with a zeroed struct none does
        assert pref.call(lib, pb.handle, LISTED, pref.opts_struct(capi, apply=1), flags=flags.data_ptr()) == 0
        assert pref.unchanged(pb, held, pref.snapshot(pb)) and pb.prune_stats() == (1, 1, 4 * B * L + REC * len(LISTED) * L)
        assert pref.call(lib, pb.handle, LISTED, o, flags=flags.data_ptr()) == 0
        assert pref.device_counts(pb).tolist() == [[0, 0], [100, 100], [0, 0]] and [pb.array[e].K for e in range(B * L)] == [0, 0, 100, 100, 0, 0]
    finally:
        pb.close()
