"""-m gpu: the evaluation engine's pose entries (pose_entries.h -> PoseEntry, pixel_math.h) against the oracle at EVERY relative
rotation between consecutive knots, 1e-11 rad up to exactly pi.

The stage API's pose kernel (k_api_poses: spline_rotation<KD, true>) is swept over the whole range by
test_gpu_stages.test_pose_chain_over_the_whole_range_of_rotations; the engine and the batched LM go through other forms of
se3_math.h -- spline_segment_eval + spline_rotation_knot_from_segs (one wave per knot), spline_rotation_knot through pose_unstaged
(k = 2, one lane), spline_rotation_from_segs / spline_rotation<KD, false> (cost-only) -- and turn the 4 x 3k quaternion Jacobian
into the tabulated R * A that sample_retire consumes.  Every other test of that code builds its knots with rot_scale <= 0.05.  The
roll-dominant scenes of roll_scenes.py keep the warps inside the keyframe at any angle (tests/test_roll_scenes.py holds the inputs
to that, on the oracle alone), so the four ways the engine makes its pose entries are compared here with the oracle at angles that
take the series branches of qlog / qexp with a non-zero angle, relative w < 0 ("flip": every odd knot negated), the |w| < 1e-10
branch of qlog ("pi") and the upper reduction ranges of fastm::atan_ratio / fastm::sincos.

Every case proves with mbavo_last_kernel / mbavo_last_layout that it reached its form (a missed witness fails).  Tolerances: the
project's -- test_gpu_fuzz._tol (1e-9 at these sizes) on every frame block relative to its largest entry, and ON TOP of it on g
and H of mbavo_eval split by parameter kind (translation [0, 3N), rotation [3N, 6N): the layout of merge_hessian_gradient_cost),
each part relative to ITS OWN largest oracle entry, so that an error of the rotation chain cannot hide under larger entries;
valid counts exact; cost-only cost within the tolerance of the oracle's and 1e-11 of the H/g pass's; per-patch costs the oracle's
bits up to max(2, 1 %) entries, none off by more than 1e-5 (test_gpu_fuzz).  Between forms on the same scene: the lane-per-pixel
prologue and the pose kernel give identical bits; every other pair agrees within test_gpu_schedules._group_tol.

Worst observed relative difference from the oracle per angle and form (MI355X; the largest over both knot signs, k = 2 and 4 and
every shape, of: each frame block, the two parts of g, the three parts of H, the cost and the cost-only cost).  Per-patch costs
were the oracle's bits in every case (no mismatch at all).
    angle    pose kernel  prologue   sp one launch  sp three launches
    1e-11    4.3e-16      4.3e-16    4.3e-16        2.3e-16
    1e-9     9.5e-16      9.5e-16    9.5e-16        9.5e-16
    3e-6     1.5e-15      1.5e-15    1.6e-15        1.5e-15
    1e-3     1.8e-15      1.8e-15    2.4e-15        1.6e-15
    0.05     2.0e-15      2.0e-15    2.3e-15        1.9e-15
    0.4      1.7e-15      1.7e-15    2.1e-15        2.0e-15
    1.1      1.9e-15      1.3e-15    1.2e-15        1.2e-15
    2.2      1.5e-15      1.5e-15    1.4e-15        1.4e-15
    2.9      1.4e-15      1.4e-15    1.8e-15        1.2e-15
    3.1      1.9e-15      1.1e-15    2.5e-10 (*)    2.5e-10 (*)
    pi       4.3e-15      2.1e-15    2.1e-15        1.9e-15
(*) one scene (k = 4, S = 16, 3.1 rad, flip; only the sample-parallel rows run S = 16): g_t 2.1e-10, g_R 2.5e-10, H parts 5e-12 to
8e-12, frame block 1.1e-11, costs and per-patch costs exact.  It is not the pose chain: the pose entries of a frame are shared by all
its pixels, and with the 80 keypoints evaluated as 80 one-keypoint problems 239 of the 240 (keypoint, frame) blocks are within 1e-13
and one (keypoint 33, frame 2) is off by 7e-9, translation and rotation columns alike, under the lane-per-pixel kernel with either
pose form as well -- the one-ulp fp32 bilinear weight of test_gpu_fuzz._tol (a tap whose intensity blend does not move and whose
gradient blend does), at the size that docstring derives (~1e-7 of one pixel's row among 1920 residuals).  Everything else: 4.3e-15.
"""
import ctypes as C

import numpy as np
import pytest

import eval_support as es
import lm_support as lms
import roll_scenes
import scenes
from roll_scenes import ANGLES, angle_id

pytestmark = pytest.mark.gpu

F = 3  # frames at capture times 0.25, 0.75, 1.25: segments idx = 0, 1, 2 of the 2 + k knots
FEW = [1e-11, 1.1, 3.1, "pi"]  # the angles of the shapes that do not run the whole list

# form -> engine options, and per degree (S at every angle, S at the FEW angles)
FORMS = {
    # k_pose_table: segments on waves, one wave per knot (pose_stage_b), S > kPoseSPB = 21: two workgroups per frame
    "pose_kernel": (dict(sample_parallel=-1, fused_pose=-1), {2: ((8,), (1, 21, 32)), 4: ((8,), (1, 21, 32))}),
    # the lane-per-pixel kernel's prologue: frame_pose_entries<.., STAGE2> (k = 2 staged as well), up to 21 samples
    "prologue": (dict(sample_parallel=-1, fused_pose=1, fused_pose_max_samples=21), {2: ((8,), (21,)), 4: ((8,), (21,))}),
    # sample-parallel single launch: staged for k = 4, pose_unstaged for k = 2 (S = 32: two passes of its 21-sample loop)
    "sp_one_launch": (dict(sample_parallel=1), {2: ((4,), (32,)), 4: ((4, 16), ())}),
    # sample-parallel kernel behind k_pose_table
    "sp_three_launches": (dict(sample_parallel=1, single_launch=-1), {2: ((8,), ()), 4: ((16,), ())}),
}


def _shapes(form, k, angle):
    every, few = FORMS[form][1][k]
    return every + (few if angle in FEW else ())


CASES = [(form, angle, flip, k, S) for form in FORMS for k in (2, 4) for angle in ANGLES for flip in (False, True)
         for S in _shapes(form, k, angle)]


def _case_id(c):
    form, angle, flip, k, S = c
    return "%s-k%d-S%d-%s-%s" % (form, k, S, angle_id(angle), "flip" if flip else "plain")


def _witness(form, k, S, with_h, kern, lay):
    """The kernel instantiation and layout of each form (engine.hip: Engine::evaluate)."""
    wh = "true" if with_h else "false"
    if form == "pose_kernel":
        want = "k_fused<%d,%s,false,false>" % (k, wh)
    elif form == "prologue":
        want = "k_fused<%d,%s,false,true>" % (k, wh)
        assert 0 < lay["ntiles"] <= lay["num_cus"], lay
    else:
        logs = S.bit_length() - 1
        assert 1 << logs == S and lay["sp_logs"] == logs, (S, lay)
        want = "k_fused_sp<%d,%s,false,%d,%s>" % (k, wh, logs, "true" if form == "sp_one_launch" else "false")
    assert kern == want, (form, kern, want)
    if form in ("pose_kernel", "prologue"):
        assert lay["sp_logs"] == 0, lay
    assert lay["nbf"] == F and lay["empty"] == 0 and lay["nprob"] == 1, lay


_SCENES = {}
_RUNS = {}


def _scene(orc, angle, flip, k, S):
    """The scene, its device twin and the oracle's results: once per scene, shared by every form and never modified."""
    key = (angle, flip, k, S)
    if key not in _SCENES:
        sc = roll_scenes.case_scene(angle, k, S, F, flip)
        p, keep = sc.oracle_problem(orc)
        ro, roc = orc.evaluate(p), orc.evaluate(p, with_hessian=False)
        for a in (ro["frame_blocks"], ro["patch_blocks"], ro["H"], ro["g"], roc["frame_blocks"]):
            a.setflags(write=False)
        valid = es.oracle_valid_counts(orc, sc)
        _SCENES[key] = (sc, scenes.DeviceScene(sc), ro, roc, valid)
    return _SCENES[key]


def _run(orc, ctx, form, angle, flip, k, S):
    """One scene through one form: H/g and cost-only by mbavo_eval_batch and by mbavo_eval, each with its witness."""
    key = (form, angle, flip, k, S)
    if key in _RUNS:
        return _RUNS[key]
    sc, d, ro, roc, o_valid = _scene(orc, angle, flip, k, S)
    last = lambda: (ctx.lib.mbavo_last_kernel(ctx.handle).decode(), es.layout(ctx))
    try:
        ctx.engine_opts(**FORMS[form][0])
        fb, pc, valid = scenes.gpu_eval_batch(ctx, [d], k)
        _witness(form, k, S, True, *last())
        lay = last()[1]
        fc, pcc, validc = scenes.gpu_eval_batch(ctx, [d], k, with_hessian=False)
        _witness(form, k, S, False, *last())
        ev = scenes.gpu_eval(ctx, d)
        _witness(form, k, S, True, *last())
        evc = scenes.gpu_eval(ctx, d, with_hessian=False)
        _witness(form, k, S, False, *last())
    finally:
        ctx.engine_opts()
    _RUNS[key] = dict(fb=fb, pc=pc, valid=valid, fc=fc[:, 0].copy(), pcc=pcc, validc=validc, H=ev["H"], g=ev["g"], cost=ev["cost"],
                      cost_c=evc["cost"], lay=lay, kern=_kernel_name(form, k, S, True), kern_c=_kernel_name(form, k, S, False))
    return _RUNS[key]


def _kernel_name(form, k, S, with_h):
    wh = "true" if with_h else "false"
    if form in ("pose_kernel", "prologue"):
        return "k_fused<%d,%s,false,%s>" % (k, wh, "true" if form == "prologue" else "false")
    return "k_fused_sp<%d,%s,false,%d,%s>" % (k, wh, S.bit_length() - 1, "true" if form == "sp_one_launch" else "false")


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _figures(sc, got, ro, roc):
    """Every difference from the oracle that the case asserts, relative to the largest oracle entry of the same part."""
    t, r = slice(0, 3 * sc.N), slice(3 * sc.N, 6 * sc.N)
    fig = {"fb": max(_rel(got["fb"][f], ro["frame_blocks"][f]) for f in range(sc.F)),
           "g_t": _rel(got["g"][t], ro["g"][t]), "g_R": _rel(got["g"][r], ro["g"][r]),
           "H_tt": _rel(got["H"][t, t], ro["H"][t, t]), "H_tR": _rel(got["H"][t, r], ro["H"][t, r]),
           "H_RR": _rel(got["H"][r, r], ro["H"][r, r]),
           "cost": abs(got["cost"] - ro["cost"]) / abs(ro["cost"]),
           "fc": max(abs(got["fc"][f] - roc["frame_blocks"][f, 0]) / abs(roc["frame_blocks"][f, 0]) for f in range(sc.F)),
           "cost_c": abs(got["cost_c"] - roc["cost"]) / abs(roc["cost"])}
    want_pc = ro["patch_blocks"][:, :, 0].ravel()
    fig["pc_mismatches"] = int((got["pc"] != want_pc).sum())
    fig["pc"] = _rel(got["pc"], want_pc)
    return fig


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_pose_entries_match_oracle(orc, mbavo, gpu_ctx, case):
    form, angle, flip, k, S = case
    sc, d, ro, roc, o_valid = _scene(orc, angle, flip, k, S)
    got = _run(orc, gpu_ctx, form, angle, flip, k, S)
    fig = _figures(sc, got, ro, roc)
    print("pose_entries_figures %s %s" % (_case_id(case), " ".join("%s=%.3g" % kv for kv in sorted(fig.items()))))
    # the inputs: (nearly) every warp inside the keyframe; the same pixels valid as in the oracle, in both passes
    assert o_valid.min() >= 0.9 * sc.K * sc.P, o_valid
    assert np.array_equal(got["valid"], o_valid) and np.array_equal(got["validc"], o_valid), (got["valid"], o_valid)
    tol = es.tol(sc)
    for part in ("fb", "g_t", "g_R", "H_tt", "H_tR", "H_RR", "cost", "fc", "cost_c"):
        assert fig[part] <= tol, (part, fig)
    assert np.array_equal(got["H"], got["H"].T)
    # the cost-only pass (WITH_J = false forms of the pose chain) against the H/g pass
    scale = max(np.abs(got["fb"][:, 0]).max(), 1e-300)
    assert np.abs(got["fc"] - got["fb"][:, 0]).max() <= 1e-11 * scale, (got["fc"], got["fb"][:, 0])
    assert abs(got["cost_c"] - got["cost"]) <= 1e-11 * abs(got["cost"])
    # per-patch costs: the oracle's bits up to rare one-ulp fp32 weight flips (test_gpu_fuzz)
    assert fig["pc_mismatches"] <= max(2, int(0.01 * got["pc"].size)), fig
    assert fig["pc"] <= 1e-5, fig


BITS = [(angle, flip, k, S) for k in (2, 4) for angle in ANGLES for flip in (False, True) for S in _shapes("prologue", k, angle)]


@pytest.mark.parametrize("angle,flip,k,S", BITS, ids=["k%d-S%d-%s-%s" % (k, S, angle_id(a), "flip" if f else "plain") for a, f, k, S in BITS])
def test_prologue_equals_pose_kernel_at_every_angle(orc, mbavo, gpu_ctx, angle, flip, k, S):
    """test_gpu_fused.test_pose_prologue_equals_pose_kernel's claim -- the same arithmetic per entry, so identical frame blocks,
    per-patch costs and valid counts, H/g and cost-only -- beyond its small rotations."""
    a = _run(orc, gpu_ctx, "prologue", angle, flip, k, S)
    b = _run(orc, gpu_ctx, "pose_kernel", angle, flip, k, S)
    assert a["kern"].endswith(",true>") and b["kern"].endswith(",false>") and a["lay"] == b["lay"]
    for key in ("fb", "pc", "valid", "fc", "pcc", "validc", "H", "g", "cost", "cost_c"):
        assert np.array_equal(a[key], b[key]), key


def _pairs():
    out = []
    for k in (2, 4):
        for angle in ANGLES:
            for flip in (False, True):
                by_S = {}
                for form in FORMS:
                    for S in _shapes(form, k, angle):
                        by_S.setdefault(S, []).append(form)
                for S, forms in sorted(by_S.items()):
                    out += [(angle, flip, k, S, fa, fb) for i, fa in enumerate(forms) for fb in forms[i + 1:]
                            if (fa, fb) != ("pose_kernel", "prologue")]
    return out


PAIRS = _pairs()


@pytest.mark.parametrize("angle,flip,k,S,form_a,form_b", PAIRS,
                         ids=["%s-%s-k%d-S%d-%s-%s" % (fa, fb, k, S, angle_id(a), "flip" if f else "plain") for a, f, k, S, fa, fb in PAIRS])
def test_forms_agree_on_the_same_scene(orc, mbavo, gpu_ctx, angle, flip, k, S, form_a, form_b):
    """Two forms of the pose entries (and the kernels behind them) on one scene: the same valid pixels, frame blocks within the
    grouping bound of the tile sums, per-patch costs identical where the per-pixel kernel is the same and 1e-12 otherwise."""
    a = _run(orc, gpu_ctx, form_a, angle, flip, k, S)
    b = _run(orc, gpu_ctx, form_b, angle, flip, k, S)
    assert np.array_equal(a["valid"], b["valid"]) and np.array_equal(a["validc"], b["validc"])
    gtol = es.group_tol(max(a["lay"]["max_slot_tiles"], b["lay"]["max_slot_tiles"]))
    for f in range(F):
        scale = np.abs(b["fb"][f]).max()
        assert np.abs(a["fb"][f] - b["fb"][f]).max() <= gtol * scale, (f, np.abs(a["fb"][f] - b["fb"][f]).max() / scale)
        assert abs(a["fc"][f] - b["fc"][f]) <= gtol * max(abs(b["fc"][f]), scale), f
    for key, kk in (("pc", "kern"), ("pcc", "kern_c")):
        if es.per_pixel_kernel(a[kk]) == es.per_pixel_kernel(b[kk]):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert np.abs(a[key] - b[key]).max() <= 1e-12 * max(np.abs(b[key]).max(), 1e-300), key


def test_matrix_reaches_every_form_and_branch():
    """The matrix as a whole: every form runs every angle with both knot signs at k = 2 and 4, and the knots of those scenes take every
    branch of qlog (restated in roll_scenes.branches)."""
    for form in FORMS:
        for k in (2, 4):
            assert {(a, f) for fo, a, f, kk, S in CASES if fo == form and kk == k} == {(a, f) for a in ANGLES for f in (False, True)}
    seen = set()
    for form, angle, flip, k, S in CASES:
        seen |= set(roll_scenes.branches(roll_scenes.case_scene(angle, k, S, F, flip)))
    assert seen == {"series", "general+", "general-", "pi"}, seen


LM_CASES = [(4, 6, 1, 4, 1.1), (4, 6, 1, 4, 3.1), (4, 6, 1, 4, "pi"), (2, 4, 2, 4, 1.1), (2, 4, 2, 4, 3.1), (2, 4, 2, 4, "pi"),
            (4, 6, 1, 32, 3.1)]  # S = 32 at k = 4: frame_pose_entries makes two passes with its barrier between them


@pytest.mark.parametrize("k,N,F_,S,angle", LM_CASES, ids=["k%d-N%d-F%d-S%d-%s" % (k, N, F_, S, angle_id(a)) for k, N, F_, S, a in LM_CASES])
def test_lm_batch_pose_entries_same_bits_on_roll_splines(mbavo, gpu_ctx, k, N, F_, S, angle):
    """test_gpu_schedules.test_lm_batch_pose_entries_same_bits (rot_scale = 0.05) on the same problems with every pair's rotation
    knots replaced by a roll spline (odd pairs with alternating knot signs): the solve launch's pose entries (pose_entries = 0) and
    the evaluation's pose launch (-1) give identical records, final knots and results, and steps are taken."""
    import torch
    from mba_vo_amd import workloads
    capi = mbavo.capi
    kR = lambda b: roll_scenes.roll_knots(N, angle, np.random.default_rng([41, b]), flip=bool(b % 2))
    out = {}
    for pe in (0, -1):
        probs = lms.scene(12, k, N, F_, seed=41, S=S, kR=kR)
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
    assert repr(out[0]) == repr(out[-1]), (k, N, F_, S, angle)
    assert sum(r[1] for r in out[0][2]) > 0, (k, N, F_, S, angle)  # steps were taken
