"""The step of a batch of keyframe pairs from frame to frame (mbavo_pairs_assess, mbavo_pairs_update,
mbavo_spline_transform_by_right): what can be held without a GPU.  The entry points exist in the library, the header and the
binding; the assessment struct's mirror has the library's size; TransformByRight equals the oracle's; and the inputs of the GPU
checks (tests/test_gpu_pairs_step.py) are good ones by the oracle's own answers: both keyframe verdicts occur, no average lies
within the comparison's bound of a threshold, and on the six teacher-forced sequences the verdict alternates with the margins
the GPU file relies on."""
import ctypes as C
import os
import re

import numpy as np

import frontend
import pairs_step as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_assessment_size", "mbavo_pairs_assess", "mbavo_pairs_assess_stats", "mbavo_pairs_update", "mbavo_pairs_update_stats",
       "mbavo_spline_transform_by_right"]
E_ARG = -1


def test_step_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_pairs_assessment_size() == C.sizeof(capi.PairsAssessment) == 88
    assert lib.mbavo_sizeof(10) == -1 and lib.mbavo_abi_version() == 3  # (its own size entry point: no new mbavo_sizeof index)


def test_null_arguments(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    out3 = (C.c_longlong * 3)()
    a = (capi.PairsAssessment * 1)()
    assert lib.mbavo_pairs_assess(None, 2.5, 6.0, 3.0, a) == E_ARG
    assert lib.mbavo_pairs_assess_stats(None, out3) == E_ARG and lib.mbavo_pairs_update_stats(None, out3) == E_ARG
    assert lib.mbavo_pairs_update(None, None, 0, None, None, None, None) == E_ARG
    kt, kR, q, t = np.zeros(6), np.zeros(8), np.array([0.0, 0, 0, 1]), np.zeros(3)
    dp = capi.dp
    assert lib.mbavo_spline_transform_by_right(None, dp(kR), 2, dp(q), dp(t)) == E_ARG
    assert lib.mbavo_spline_transform_by_right(dp(kt), None, 2, dp(q), dp(t)) == E_ARG
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), 2, None, dp(t)) == E_ARG
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), 2, dp(q), None) == E_ARG
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), -1, dp(q), dp(t)) == E_ARG


def test_transform_by_right_matches_oracle(mbavo, orc):
    """SplineSE3::TransformByRight through the C ABI against orc_spline_transform_by_right on random knots, with the tolerances
    tests/test_host_logic.py holds the sibling mbavo_spline_transform_to to: 1e-13 on the translations, 1e-14 on the quaternions
    (knots of unit size); the identity leaves the knots as they are, bit for bit."""
    lib, L, dp = mbavo.load(), orc.lib(), mbavo.capi.dp
    rng = np.random.default_rng(11)
    for N in (1, 2, 4, 16):
        for scale in (1e-6, 0.05, 1.0):
            kt = rng.normal(0, 1, 3 * N)
            kR = rng.normal(0, 1, (N, 4))
            kR = np.ascontiguousarray((kR / np.linalg.norm(kR, axis=1, keepdims=True)).ravel())
            d = np.zeros(7)
            assert lib.mbavo_se3_exp(dp(rng.normal(0, 1, 6) * scale), dp(d)) == 0
            q, t = np.ascontiguousarray(d[3:]), np.ascontiguousarray(d[:3])
            kt2, kR2, kt0, kR0 = kt.copy(), kR.copy(), kt.copy(), kR.copy()
            assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), N, dp(q), dp(t)) == 0
            L.orc_spline_transform_by_right(orc.dp(kt2), orc.dp(kR2), N, orc.dp(q), orc.dp(t))
            assert np.abs(kt - kt2).max() < 1e-13 and np.abs(kR - kR2).max() < 1e-14, (N, scale)
            assert np.abs(kt - kt0).max() > 0.1 * scale * 1e-3 and np.abs(kR - kR0).max() > 0  # (it moved)
    kt, kR = rng.normal(0, 1, 12), rng.normal(0, 1, 16)
    kt0, kR0 = kt.copy(), kR.copy()
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), 4, dp(np.array([0.0, 0, 0, 1])), dp(np.zeros(3))) == 0
    assert np.array_equal(kt, kt0) and np.array_equal(kR, kR0)


def test_assess_inputs_have_margin(orc):
    """The inputs of the GPU file's check 1 by the oracle alone (keypoints from the numpy restatement of the prepare): every
    pair's averages lie further than the comparison's bound from every threshold, both verdicts occur, and all three ways to a
    verdict are taken: past flow_mag1; past flow_mag0 with a short blur kernel; past flow_mag0 but not a keyframe because the blur
    kernel is long.  The absolute floor of the bound is re-measured against the oracle's FMA build where that exists."""
    seen = set()
    for (B, H, W, k) in ps.ASSESS_CASES:
        case = ps.assess_inputs(B, H, W, k)
        verdicts = []
        for b, (xy, z) in enumerate(ps.host_keypoints0(case, 4)):
            assert len(z) > 50
            v, af, ak = ps.oracle_assess(orc, case["intr"], xy, z, k, case["t0"][b], case["dt"], case["kt"][b], case["kR"][b], case["cap"][b], case["exp"][b])
            assert ps.margin_ok(af, ak), (B, H, W, b, af, ak)
            verdicts.append(v)
            seen.add("flow1" if af > ps.FLOW1 else ("flow0" if v else ("kernel" if af > ps.FLOW0 else "rest")))
        assert B == 1 or set(verdicts) == {0, 1}, (B, H, W)
    assert seen == {"flow1", "flow0", "kernel", "rest"}, seen
    fma = orc.fma_variant()
    if fma is not None:
        worst = ps.identity_motion_noise(orc, fma)
        assert max(worst) <= ps.MEASURED_FMA_NOISE, worst  # (the figure the floor is made from still holds)


def test_sequences_alternate_with_margin(orc):
    """The six sequences of the GPU file's check 7 through the oracle's trackFrame: over the eight tracked frames the keyframe
    verdict alternates 0, 1, 0, 1, ..., so an update has listed and unlisted pairs on every other frame; avg_flow stays at least
    0.15 px from both flow thresholds (closest: 2.343 against 2.5) and avg_kernel at most 2.05 against 3.0 -- far more than a 1e-4
    knot difference moves them."""
    closest, kernel_max = np.inf, 0.0
    for s in ps.SEQ_SEEDS:
        seq = frontend.make_sequence(orc, M=ps.SEQ_M, seed=s)
        out = frontend.run_oracle_vo(orc, seq, frontend.DEFAULTS)
        assert [o["is_keyframe"] for o in out[1:]] == [0, 1] * (ps.SEQ_M // 2), s
        for o in out[1:]:
            closest = min(closest, abs(o["avg_flow"] - ps.FLOW0), abs(o["avg_flow"] - ps.FLOW1))
            kernel_max = max(kernel_max, o["avg_kernel"])
        tol = ps.knot_pixel_bound(seq["intr"])
    assert closest >= 0.15 and kernel_max <= 2.05, (closest, kernel_max)
    assert closest > 10 * tol and ps.KERNEL - kernel_max > 10 * tol
