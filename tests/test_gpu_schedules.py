"""-m gpu: the evaluation engine's scheduling options (mbavo_engine_opts, include/mbavo.h) and the option tails of the LM loops,
each against the oracle and against the default schedule of the same input.

Every branch of the engine's decision tree (Engine::rebuild_layout: tiling, sample-parallel or lane-per-pixel kernel, flat or tree
finalize; Engine::evaluate: single launch with the ticket epilogue or separate launches, pose prologue fused or not) sums the tile
partials in its own code.  The matrix below runs every list through every schedule and proves with mbavo_last_kernel and
mbavo_last_layout which branch each case reached: a case whose witness fails is a failing test, not a skip.

Tolerances:
- oracle: 1e-9 relative on the packed frame blocks, or test_gpu_fuzz._tol for tiny problems; valid-pixel counts exact;
- against the default schedule of the same list: valid counts identical; frame blocks within the grouping bound of es.group_tol
  (only the grouping of the tile sums changes); per-patch costs identical bit for bit whenever the per-pixel kernel is the same
  (a tile is a range of whole keypoints, so no patch is split between tiles), 1e-12 between the sample-parallel and the
  lane-per-pixel kernel (another order of the sums over a patch's pixels and samples: the fuzz bound);
- mbavo_eval_batch_merged: bit-identical to mbavo_eval_batch + mbavo_merge_device under every schedule."""
import ctypes as C

import numpy as np
import pytest

import eval_support as es
import lm_support as lms
import scenes

pytestmark = pytest.mark.gpu


SMALL = dict(trans_scale=0.002, rot_scale=0.02)  # S = 32: blur samples stay on the spline
# name -> (spline degree, scene keyword lists, gradient format: 0 float, 1 IEEE half, 2 packed keyframe)
LISTS = {
    "k2_S4": (2, [dict(S=4, F=1, k=2, P=8, K=145, seed=1)], 0),
    "k2_S8_F2": (2, [dict(S=8, F=2, k=2, P=8, K=300, seed=2)], 0),
    "k2_S16": (2, [dict(S=16, F=1, k=2, P=8, K=200, seed=3)], 0),
    "k2_S32": (2, [dict(S=32, F=1, k=2, P=8, K=60, seed=4, **SMALL)], 0),
    "k4_S4_P3_F2": (4, [dict(S=4, F=2, k=4, P=3, K=77, seed=5)], 0),
    "k4_S8": (4, [dict(S=8, F=1, k=4, P=8, K=145, seed=6)], 0),
    "k4_S16_F3": (4, [dict(S=16, F=3, k=4, P=8, K=500, seed=7)], 0),
    "k4_S32_F2": (4, [dict(S=32, F=2, k=4, P=8, K=60, seed=8, **SMALL)], 0),
    "k4_S12": (4, [dict(S=12, F=2, k=4, P=8, K=145, seed=9)], 0),
    "k2_S21": (2, [dict(S=21, F=1, k=2, P=5, K=97, seed=10)], 0),
    "k4_with_K0": (4, [dict(S=4, F=2, k=4, P=8, K=60, seed=11), dict(S=4, F=2, k=4, P=8, K=0, seed=12),
                       dict(S=4, F=1, k=4, P=3, K=1, seed=13)], 0),
    "k2_dense_60x80_S1": (2, [dict(H=60, W=80, S=1, F=1, k=2, P=1, kp="dense", margin=0, seed=14)], 0),
    "k4_dense_120x160_S8": (4, [dict(H=120, W=160, S=8, F=1, k=4, P=1, kp="dense", margin=0, seed=15)], 0),
    "k4_flat_70": (4, [dict(S=8, F=1 + (i % 2), k=4, P=8, K=5 + (7 * i) % 36, seed=500 + i) for i in range(70)], 0),
    "k4_packed_S8": (4, [dict(S=8, F=2, k=4, P=8, K=145, seed=16)], 2),
    "k2_packed_dense_S4": (2, [dict(H=60, W=80, S=4, F=1, k=2, P=1, kp="dense", margin=0, seed=17)], 2),
    "k4_fp16_S16": (4, [dict(S=16, F=1, k=4, P=8, K=200, seed=18)], 1),
    "k2_fp16_S8_F3": (2, [dict(S=8, F=3, k=2, P=8, K=145, seed=19)], 1),
}

SCHEDULES = {
    "default": {},
    "sp_on": dict(sample_parallel=1),
    "sp_off": dict(sample_parallel=-1),
    "three_launches": dict(single_launch=-1),
    "pose_kernel": dict(fused_pose=-1),
    "prologue_max_S1": dict(fused_pose_max_samples=1),
    "prologue_max_S21": dict(fused_pose_max_samples=21),
    "tiles_per_cu2": dict(tiles_per_cu=2),
    "tiles_per_cu4": dict(tiles_per_cu=4),
    "tiles_per_cu16": dict(tiles_per_cu=16),
    "min_tile_px1": dict(min_tile_pixels=1),
    "min_tile_px_huge": dict(min_tile_pixels=1 << 20),
    "sp_slot_tiles1": dict(sp_max_slot_tiles=1),
    "sp_slot_tiles4096": dict(sp_max_slot_tiles=4096),
    # several rounds of lane-per-pixel workgroups on lists far smaller than 256 tiles of 256 pixels
    "tiles_per_cu16_min_tile_px1": dict(tiles_per_cu=16, min_tile_pixels=1),
}


def _model(k, scs, fmt, opts, num_cus):
    """The layout and kernel each schedule must reach, restated from the engine's rules (engine.hip: rebuild_layout, evaluate)."""
    tpc = opts.get("tiles_per_cu") or 1
    min_px = opts.get("min_tile_pixels") or 256
    slot_tiles = opts.get("sp_max_slot_tiles") or 64
    sp = opts.get("sample_parallel", 0)
    sp_waves = 8
    target = num_cus * tpc
    pixels = sum(sc.F * sc.K * sc.P for sc in scs)

    def kpt(ppt, P):
        return max(1, ppt // P)

    def count(ppt):
        return sum(sc.F * -(-sc.K // kpt(ppt, sc.P)) for sc in scs)

    S0 = scs[0].S
    lg = max(0, (S0 - 1).bit_length())
    logs = 0
    if (1 << lg) == S0 and 2 <= lg <= 5 and all(sc.S == S0 for sc in scs) and fmt == 0 and sp >= 0:
        if sp > 0 or pixels <= 2 * sp_waves * (64 >> lg) * num_cus:
            logs = lg

    def tile_px(lg_):
        lo = sp_waves * (64 >> lg_) if lg_ else min_px
        hi = max(pixels, lo)
        if count(lo) > target:
            while lo < hi:
                mid = (lo + hi) // 2
                if count(mid) <= target:
                    hi = mid
                else:
                    lo = mid + 1
        return lo

    ppt = tile_px(logs)
    if logs and sp <= 0:
        lanes = 4 if k == 2 else 1
        if max(-(-sc.K // kpt(ppt, sc.P)) for sc in scs) > slot_tiles * lanes:
            logs, ppt = 0, tile_px(0)
    per_slot = [-(-sc.K // kpt(ppt, sc.P)) for sc in scs for _ in range(sc.F)]
    lay = dict(ntiles=sum(per_slot), nbf=len(per_slot), max_slot_tiles=max(per_slot), sp_logs=logs,
               flat=int(len(per_slot) >= 64 and max(per_slot) <= 4), empty=int(min(per_slot) == 0), num_cus=num_cus, nprob=len(scs))
    one = logs > 0 and (logs <= 5 if k == 2 else logs <= 4) and not lay["empty"] and opts.get("single_launch", 0) >= 0
    max_S = max(sc.S for sc in scs)
    fused = (lay["ntiles"] <= num_cus and max_S <= (opts.get("fused_pose_max_samples") or 8) and max_S <= 21
             and opts.get("fused_pose", 0) >= 0 and not one and logs == 0 and lay["ntiles"] > 0)

    def kernel(with_h):
        wh = "true" if with_h else "false"
        if logs:
            return "k_fused_sp<%d,%s,false,%d,%s>" % (k, wh, logs, "true" if one else "false")
        g = "packed" if fmt == 2 and with_h else ("true" if fmt == 1 else "false")
        return "k_fused<%d,%s,%s,%s>" % (k, wh, g, "true" if fused else "false")

    return lay, kernel(True), kernel(False), one, fused


_CACHE = {}


def _list_data(orc, mbavo, gpu_ctx, name):
    """Scenes, device twins, oracle results and the default schedule's run of one list: computed once per list."""
    if name in _CACHE:
        return _CACHE[name]
    k, kws, fmt = LISTS[name]
    scs = []
    for kw in kws:
        sc = scenes.Scene(**dict(kw, K=max(kw.get("K", 145), 1)))
        if kw.get("K", 1) == 0:  # no keypoint survived detection
            sc.kp_xy, sc.kp_z, sc.K = np.zeros((0, 2)), np.zeros(0), 0
        scs.append(sc)
    ds = [scenes.DeviceScene(sc, packed=fmt == 2, half=fmt == 1) for sc in scs]
    for i, sc in enumerate(scs):  # zero-length device tensors have a null data_ptr: give an empty problem valid (unused) pointers
        if sc.K == 0:
            j = next(j for j, o in enumerate(scs) if o.K > 0)
            ds[i].kp_xy_ptr, ds[i].kp_z = ds[j].kp_xy_ptr, ds[j].kp_z
    oracle = []
    for sc in scs:
        if sc.K == 0:
            oracle.append(None)
            continue
        p, keep = sc.oracle_problem(orc)
        ro, roc = orc.evaluate(p), orc.evaluate(p, with_hessian=False)
        oracle.append((ro["frame_blocks"].reshape(sc.F, sc.E), roc["frame_blocks"].reshape(sc.F, sc.E)[:, 0],
                       es.oracle_valid_counts(orc, sc)))
    gpu_ctx.engine_opts()
    base = es.run(mbavo, gpu_ctx, k, scs, ds)
    _CACHE[name] = (k, scs, ds, fmt, oracle, base)
    return _CACHE[name]


def _regime(name, sched, lay, kern, k, scs):
    """What the named (list, schedule) cases exist for, beyond the restated rules of _model."""
    S = max(sc.S for sc in scs)
    if sched == "sp_on" and name in ("k4_dense_120x160_S8",):
        # the ticket epilogue over hundreds of partials: the single launch with far more than 16 tiles per lane in one slot
        assert kern.startswith("k_fused_sp<") and kern.endswith(",true>") and lay["max_slot_tiles"] > 16 * (4 if k == 2 else 1), (kern, lay)
    if sched == "sp_slot_tiles4096" and name == "k4_dense_120x160_S8":
        assert kern.startswith("k_fused_sp<") and kern.endswith(",true>") and lay["max_slot_tiles"] > 64, (kern, lay)
    if sched == "prologue_max_S21" and name in ("k4_S12", "k2_S21", "k4_fp16_S16"):
        assert kern.startswith("k_fused<") and kern.endswith(",true>") and S > 8, kern  # the fused prologue with 9 .. 21 samples
    if sched == "tiles_per_cu16_min_tile_px1" and name in ("k4_dense_120x160_S8", "k4_S16_F3", "k2_dense_60x80_S1"):
        assert lay["ntiles"] > lay["num_cus"] and kern.startswith("k_fused<") and kern.endswith(",false>"), (kern, lay)  # several rounds
    if (sched == "min_tile_px1" and name in ("k4_fp16_S16", "k2_S21")) or (sched == "tiles_per_cu16_min_tile_px1" and name in ("k4_S12", "k4_packed_S8")):
        assert lay["ntiles"] == sum(sc.F * sc.K for sc in scs), lay  # one keypoint per tile
    if sched == "min_tile_px_huge" and not lay["sp_logs"]:
        assert lay["ntiles"] == sum(sc.F for sc in scs if sc.K > 0), lay  # one tile per slot
    if name == "k4_flat_70":
        assert lay["flat"] == (lay["max_slot_tiles"] <= 4) and lay["nbf"] >= 64, lay
    if name == "k4_with_K0":  # a slot without tiles: no workgroup would finalize it in the single launch
        assert lay["empty"] == 1 and not (kern.startswith("k_fused_sp<") and kern.endswith(",true>")), (kern, lay)


CASES = [(n, s) for n in LISTS for s in SCHEDULES]


@pytest.mark.parametrize("name,sched", CASES, ids=["%s-%s" % c for c in CASES])
def test_schedule_matrix(orc, mbavo, gpu_ctx, name, sched):
    k, scs, ds, fmt, oracle, base = _list_data(orc, mbavo, gpu_ctx, name)
    opts = SCHEDULES[sched]
    try:
        gpu_ctx.engine_opts(**opts)
        got = es.run(mbavo, gpu_ctx, k, scs, ds)
    finally:
        gpu_ctx.engine_opts()
    # witness: the layout and the kernels the engine's rules give for this list under this schedule, and the case's own regime
    lay, kern_h, kern_c, one, fused = _model(k, scs, fmt, opts, got["lay"]["num_cus"])
    assert got["lay"] == lay and got["lay_c"] == lay and got["lay_m"] == lay, (got["lay"], lay)
    assert (got["kern"], got["kern_c"], got["kern_m"]) == (kern_h, kern_c, kern_h)
    _regime(name, sched, got["lay"], got["kern"], k, scs)
    # oracle, problem by problem
    row = 0
    for sc, want in zip(scs, oracle):
        rows = slice(row, row + sc.F)
        row += sc.F
        if want is None:  # K = 0: all-zero blocks and counts
            assert not got["fb"][rows].any() and not got["valid"][rows].any() and not got["fc"][rows].any()
            continue
        fbo, fco, vo = want
        tol = es.tol(sc)
        assert np.abs(got["fb"][rows] - fbo).max() <= tol * np.abs(fbo).max(), (name, sched)
        assert np.abs(got["fc"][rows] - fco).max() <= tol * max(np.abs(fco).max(), 1e-300), (name, sched)
        assert np.array_equal(got["valid"][rows], vo) and np.array_equal(got["validc"][rows], vo)
    # against the default schedule of the same list: only the grouping of the tile sums may change
    assert np.array_equal(got["valid"], base["valid"]) and np.array_equal(got["validc"], base["validc"])
    gtol = es.group_tol(max(got["lay"]["max_slot_tiles"], base["lay"]["max_slot_tiles"]))
    for r in range(got["fb"].shape[0]):
        scale = np.abs(base["fb"][r]).max()
        assert np.abs(got["fb"][r] - base["fb"][r]).max() <= gtol * scale, (name, sched, r)
        assert abs(got["fc"][r] - base["fc"][r]) <= gtol * max(abs(base["fc"][r]), scale), (name, sched, r)
    # per-patch costs: a tile is a range of whole keypoints, so the same per-pixel kernel gives the same bits
    for key, kk, bk in (("pc", got["kern"], base["kern"]), ("pcc", got["kern_c"], base["kern_c"])):
        if es.per_pixel_kernel(kk) == es.per_pixel_kernel(bk):
            assert np.array_equal(got[key], base[key]), (name, sched, key, kk, bk)
        else:
            assert np.abs(got[key] - base[key]).max() <= 1e-12 * max(np.abs(base[key]).max(), 1e-300), (name, sched, key, kk, bk)
    # mbavo_eval_batch_merged == mbavo_eval_batch + mbavo_merge_device, and the frame blocks it leaves are the plain ones
    assert np.array_equal(got["fb_m"], got["fb"]) and np.array_equal(got["sys_m"], got["sys_a"]), (name, sched)


def test_schedule_matrix_reaches_every_regime(orc, mbavo, gpu_ctx):
    """The matrix as a whole: every branch of the decision tree is taken by at least one case (by the rules of _model, which
    test_schedule_matrix holds every case's reported layout and kernels to)."""
    seen = set()
    for name, sched in CASES:
        k, scs, ds, fmt, oracle, base = _list_data(orc, mbavo, gpu_ctx, name)
        num_cus = base["lay"]["num_cus"]
        lay, kern, _, one, fused = _model(k, scs, fmt, SCHEDULES[sched], num_cus)
        seen.add("sp_one" if one else ("sp_three" if lay["sp_logs"] else ("lpp_fused" if fused else "lpp_pose_kernel")))
        seen.add("flat" if lay["flat"] else "tree")
        if one and lay["max_slot_tiles"] > 16 * (4 if k == 2 else 1):
            seen.add("ticket_many_partials")
        if fused and max(sc.S for sc in scs) > 8:
            seen.add("prologue_S_above_8")
        if not lay["sp_logs"] and lay["ntiles"] > num_cus:
            seen.add("lpp_rounds")
        if lay["ntiles"] == sum(sc.F * sc.K for sc in scs) and max(sc.K for sc in scs) > 1:
            seen.add("one_keypoint_per_tile")
        if lay["ntiles"] == lay["nbf"] - sum(sc.F for sc in scs if sc.K == 0) and max(sc.K * sc.P for sc in scs) > 256:
            seen.add("one_tile_per_slot")
        if lay["empty"]:
            seen.add("empty_slot")
    want = {"sp_one", "sp_three", "lpp_fused", "lpp_pose_kernel", "flat", "tree", "ticket_many_partials", "prologue_S_above_8",
            "lpp_rounds", "one_keypoint_per_tile", "one_tile_per_slot", "empty_slot"}
    assert want <= seen, want - seen


PROLOGUE_LISTS = ["k4_S12", "k2_S21", "k4_S16_F3", "k2_S16", "k4_fp16_S16"]


@pytest.mark.parametrize("name", PROLOGUE_LISTS)
def test_pose_prologue_equals_pose_kernel_above_8_samples(orc, mbavo, gpu_ctx, name):
    """fused_pose_max_samples = 21 lets the lane-per-pixel kernel's pose prologue run for up to kPoseSPB = 21 samples (and
    sample_parallel = -1 keeps power-of-two S off the sample-parallel kernel): its entries are the pose kernel's, entry by entry, so
    frame blocks, per-patch costs and valid counts are IDENTICAL to fused_pose = -1, H/g and cost-only.  Extends
    test_gpu_fused.test_pose_prologue_equals_pose_kernel (S <= 8) to the 9 .. 21 samples nothing else runs."""
    k, scs, ds, fmt, oracle, base = _list_data(orc, mbavo, gpu_ctx, name)
    runs = {}
    try:
        for mode, fp in (("fused", 1), ("kernel", -1)):
            gpu_ctx.engine_opts(sample_parallel=-1, fused_pose_max_samples=21, fused_pose=fp)
            runs[mode] = es.run(mbavo, gpu_ctx, k, scs, ds)
    finally:
        gpu_ctx.engine_opts()
    f, p = runs["fused"], runs["kernel"]
    assert f["kern"].endswith(",true>") and f["kern_c"].endswith(",true>") and p["kern"].endswith(",false>"), (f["kern"], p["kern"])
    assert f["lay"]["ntiles"] <= f["lay"]["num_cus"] and f["lay"]["sp_logs"] == 0 and max(sc.S for sc in scs) > 8, f["lay"]
    for key in ("fb", "pc", "valid", "fc", "pcc", "validc", "sys_m"):
        assert np.array_equal(f[key], p[key]), (name, key)


# ---------------------------------------------------------------------------------------------------------------------------
# Loop-level options: mbavo_track_opts (speculate, persist_levels), mbavo_vo_options.keyframe_levels_at_once, mbavo_lm_batch_opts.
# pose_entries, and the environment's override layer over mbavo_engine_opts.
TRACK_SCENES = [dict(H=120, W=160, levels=3, S=8, k=2, seed=2), dict(H=480, W=640, levels=4, S=8, k=4, F=2, seed=7)]
TRACK_VARIANTS = {
    "speculate_all": (dict(speculate=1), {}),
    "speculate_never": (dict(speculate=-1), {}),
    "per_level_kernels": (dict(persist_levels=-1), {}),
    "per_level_no_prelaunch": (dict(persist_levels=-1), dict(prelaunch=-1)),
}


def _track_close(a, b, what):
    """test_gpu_tracker.test_tracker_matches_oracle's tolerances (costs 1e-6, radius 1e-4, knots 1e-4) with the discrete trace exact."""
    assert np.array_equal(a["start"], b["start"]) and len(a["trace"]) == len(b["trace"]), what
    for x, y in zip(a["trace"], b["trace"]):
        assert x[:4] == y[:4], (what, x, y)
        assert x[4] == pytest.approx(y[4], rel=1e-4), (what, x, y)
        assert x[5] == pytest.approx(y[5], rel=1e-6, abs=1e-12) and x[6] == pytest.approx(y[6], rel=1e-6, abs=1e-12), (what, x, y)
    assert np.abs(a["kt"] - b["kt"]).max() < 1e-4 and np.abs(a["kR"] - b["kR"]).max() < 1e-4, what


@pytest.mark.parametrize("variant", sorted(TRACK_VARIANTS))
@pytest.mark.parametrize("kw", TRACK_SCENES, ids=["k2_120x160", "k4_640x480_2frames"])
def test_tracker_loop_options(orc, mbavo, gpu_ctx, kw, variant):
    """mbavo_track_opts.speculate / persist_levels (and the engine's prelaunch under per-level kernels) on the scenes of
    test_tracker_evaluation_paths_agree: the discrete trace identical to the default run, everything within the oracle tolerances.
    Speculation only decides WHICH evaluations run (a candidate evaluated with H / g stands in for the H / g evaluation at the same
    knots when the outlier flags did not change): every record, the knots and the final cost are identical bit for bit (tracker.cpp).
    Witness of the per-level path: no ride-along evaluations (they need the joint kernel of all levels), where the default of the
    k = 2 scene has some."""
    import tracking
    sc = tracking.make_tracking_scene(orc, **kw)
    st = (C.c_longlong * 3)()
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    base = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS))
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    base_posts = st[0]
    topts, eopts = TRACK_VARIANTS[variant]
    try:
        gpu_ctx.engine_opts(**eopts)
        got = tracking.run_gpu_tracker(mbavo, gpu_ctx, sc, dict(tracking.OPTS, **topts))
    finally:
        gpu_ctx.engine_opts()
    gpu_ctx.lib.mbavo_ride_along_stats(st)
    _track_close(got, base, variant)
    if variant.startswith("speculate"):
        assert got["trace"] == base["trace"] and got["cost"] == base["cost"], variant
        assert np.array_equal(got["kt"], base["kt"]) and np.array_equal(got["kR"], base["kR"]), variant
    else:
        # (the k = 4 two-frame scene's finest level takes the lane-per-pixel kernel: its default already evaluates level by level,
        # with no ride-alongs, and the option must change nothing there either)
        assert st[0] == 0 and (base_posts > 0 or kw["k"] == 4), (base_posts, list(st))
    want = tracking.run_oracle_tracker(orc, sc, dict(tracking.OPTS))
    _track_close(got, want, variant + " vs oracle")


def test_vo_loop_options_change_nothing(orc, mbavo, gpu_ctx):
    """mbavo_vo_options.keyframe_levels_at_once = -1 (pyramid, gradients and grid selection level by level), speculate = -1 and
    persist_levels = -1 on the 24-frame loop sequence of test_keyframe_preprocessing_ahead_of_the_decision_changes_nothing: every pose,
    keyframe decision, keypoint count, final keypoint set and LM record identical to the defaults, bit for bit."""
    import frontend
    from mba_vo_amd import sequence
    seq = sequence.make_sequence(gpu_ctx, H=480, W=640, M=24, trajectory="loop")
    cfg = dict(sequence.REFERENCE_CFG)
    base = frontend.run_gpu_vo(mbavo, gpu_ctx, seq, cfg)
    assert sum(f["is_keyframe"] for f in base) >= 8
    for opt in ("keyframe_levels_at_once", "speculate", "persist_levels"):
        got = frontend.run_gpu_vo(mbavo, gpu_ctx, seq, dict(cfg, **{opt: -1}))
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            assert np.array_equal(a["T"], b["T"]) and a["is_keyframe"] == b["is_keyframe"] and a["K"] == b["K"], (opt, i)
            assert a["trace"] == b["trace"], (opt, i)
        assert np.array_equal(got[-1]["kp0"][0], base[-1]["kp0"][0]) and np.array_equal(got[-1]["kp0"][1], base[-1]["kp0"][1]), opt


def test_lm_batch_pose_entries_same_bits(mbavo, gpu_ctx):
    """mbavo_lm_batch_opts.pose_entries = -1: the solve launch no longer writes the candidate's pose entries, the evaluation's pose
    launch does -- the same arithmetic (lm_batch.hip: frame_pose_entries in both), so every record and every final knot is
    identical bit for bit.  The option only acts on the wide-workgroup form (eig, n = 6N <= 48): N = 6 and 4 here."""
    import torch
    from mba_vo_amd import workloads
    capi = mbavo.capi
    for k, N, F in ((4, 6, 1), (2, 4, 2)):
        out = {}
        for pe in (0, -1):
            probs = lms.scene(12, k, N, F, seed=41)
            dw = workloads.DeviceWorkload(probs)
            o = lms.lm_batch_opts(capi, k, **dict(lms.OPTS, max_it=12))
            o.pose_entries = pe
            B, cap = len(probs), 32
            res = (capi.LmBatchResult * B)()
            trace = (capi.TraceRec * (B * cap))()
            assert gpu_ctx.lib.mbavo_lm_batch(gpu_ctx.handle, B, dw.array, C.byref(o), res, trace, cap) == 0
            torch.cuda.synchronize()
            recs = [[(t.iter, t.kind, t.num_outliers, t.radius, t.eval_cost, t.candidate_cost, t.model_change, t.quality)
                     for t in trace[b * cap:b * cap + res[b].num_trace]] for b in range(B)]
            knots = [tuple(x.cpu().numpy().tobytes() for x in dw.keep_knots(b)) for b in range(B)]
            out[pe] = (recs, knots, [(r.iterations, r.accepted, r.rejected, r.invalid, r.final_cost) for r in res])
        assert repr(out[0]) == repr(out[-1]), (k, N, F)
        assert sum(r[1] for r in out[0][2]) > 0, (k, N, F)  # steps were taken


def test_environment_override_precedence(mbavo, monkeypatch):
    """MBAVO_SP=0 in the environment overrides mbavo_engine_opts.sample_parallel = 1 (options.h: the A/B tools' layer): the context
    runs the lane-per-pixel kernel, while mbavo_get_engine_opts still returns what was set; without the variable (after
    mbavo_reload_env) the option holds again."""
    import torch
    sc = scenes.Scene(S=8, F=1, k=4, P=8, K=145, seed=6)
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.engine_opts(sample_parallel=1)
        d = scenes.DeviceScene(sc)
        monkeypatch.setenv("MBAVO_SP", "0")
        ctx.lib.mbavo_reload_env()
        fb0, _, v0 = scenes.gpu_eval_batch(ctx, [d], 4)
        kern, lay = ctx.lib.mbavo_last_kernel(ctx.handle).decode(), es.layout(ctx)
        assert kern.startswith("k_fused<") and lay["sp_logs"] == 0, (kern, lay)
        o = mbavo.capi.EngineOpts()
        assert ctx.lib.mbavo_get_engine_opts(ctx.handle, C.byref(o)) == 0 and o.sample_parallel == 1
        monkeypatch.delenv("MBAVO_SP")
        ctx.lib.mbavo_reload_env()
        fb1, _, v1 = scenes.gpu_eval_batch(ctx, [d], 4)
        kern, lay = ctx.lib.mbavo_last_kernel(ctx.handle).decode(), es.layout(ctx)
        assert kern.startswith("k_fused_sp<4,true,false,3,") and lay["sp_logs"] == 3, (kern, lay)
        assert np.array_equal(v0, v1) and np.abs(fb0 - fb1).max() <= 1e-12 * np.abs(fb1).max()
    finally:
        monkeypatch.delenv("MBAVO_SP", raising=False)
        ctx.lib.mbavo_reload_env()
        ctx.close()
