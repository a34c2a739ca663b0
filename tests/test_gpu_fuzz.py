"""Seeded random sweep of the fused evaluation against the oracle: sizes, blur samples, patch sizes, frames, spline
degree, keypoint layouts and outlier flags drawn at random, so that every kernel variant (lane-per-pixel with and
without a sample-parallel remainder round, the sample-parallel kernel, fp32 / cost-only) and the tile boundaries are hit
in combinations the hand-written cases do not list.  Tolerance as everywhere: 1e-9 relative on the packed blocks; per-patch
costs exact up to rare one-ulp fp32 weight flips (see below)."""
import numpy as np
import pytest

import eval_support as es
import scenes
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(24))
def test_random_problem_matches_oracle(orc, mbavo, gpu_ctx, seed):
    es.random_problem_matches_oracle(orc, gpu_ctx, seed)


@pytest.mark.parametrize("seed", list(range(16)) + ["checker"])
def test_random_problem_packed_keyframe_matches_float(mbavo, gpu_ctx, seed):
    """The same random problems with the keyframe handed over packed (one word per pixel, mbavo_problem.grad_fp16 = 2) and as the
    u8 image + float gradient image: every tap value is the same, so the two agree to 1e-12 relative on the packed blocks (small
    lists take the sample-parallel kernel with the float image and the lane-per-pixel kernel with the packed one: another order
    of sums), with identical valid-pixel counts; border keypoints (taps next to the zero-gradient border) included.
    "checker": the keyframe is a 0/255 checkerboard of 2 x 2 cells with salt noise, so the doubled differences in the packed word
    reach +-255 beside 0 and 255 intensities (the extremes tests/harness/tap_check.hip pins on the tap alone), with border keypoints."""
    checker = seed == "checker"
    seed = 16 if checker else seed
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.choice([2, 4]))
    S = int(rng.choice([1, 2, 3, 4, 5, 8, 16]))
    P = int(rng.choice([1, 1, 3, 8, 8, 13]))
    F = int(rng.choice([1, 1, 2, 3]))
    dense = P == 1 and rng.random() < 0.6
    kw = dict(S=S, F=F, k=k, P=P, seed=seed + 90)
    if dense:
        kw.update(H=int(rng.integers(12, 60)), W=int(rng.integers(16, 90)), kp="dense", margin=int(rng.integers(0, 3)))
    else:
        kw.update(K=int(rng.integers(1, 700)), kp=str(rng.choice(["random", "border"])))
    if rng.random() < 0.3:
        kw.update(outlier_frac=0.15)
    if checker:
        k = 4
        kw = dict(S=5, F=2, k=4, P=8, K=400, kp="border", seed=seed + 90)
    sc = scenes.Scene(**kw)
    if checker:
        yy, xx = np.mgrid[0:sc.H, 0:sc.W]
        img = np.where(((xx >> 1) + (yy >> 1)) & 1, 255, 0).astype(np.uint8)
        salt = rng.random(img.shape) < 0.02
        img[salt] = rng.integers(0, 256, int(salt.sum()), dtype=np.uint8)
        sc.ref = np.ascontiguousarray(img)
        sc.grad = synth.image_gradients(sc.ref)
        assert np.abs(sc.grad).max() == 127.5
    fb0, pc0, v0 = scenes.gpu_eval_batch(gpu_ctx, [scenes.DeviceScene(sc)], k)
    fb2, pc2, v2 = scenes.gpu_eval_batch(gpu_ctx, [scenes.DeviceScene(sc, packed=True)], k)
    assert np.array_equal(v0, v2), kw
    assert es.rel(fb2, fb0) < 1e-12, kw
    assert np.abs(pc2 - pc0).max() <= 1e-12 * max(np.abs(pc0).max(), 1e-300), kw


@pytest.mark.parametrize("seed", range(10))
def test_random_batch_matches_oracle(orc, mbavo, gpu_ctx, seed):
    """Several unrelated problems in ONE mbavo_eval_batch call (sizes, S, P and frame counts mixed, or all with the same S
    so that the sample-parallel kernel takes the list): every problem's frame blocks and patch costs must be what the
    oracle gives for that problem alone -- the offsets into the shared pose table, partials, patch costs and tiles are
    what is being exercised."""
    es.random_batch_matches_oracle(orc, gpu_ctx, seed)


@pytest.mark.parametrize("P,S", [(2, 3), (4, 5), (8, 3), (16, 3), (32, 5), (64, 3), (128, 3), (12, 3)])
def test_patch_sizes_sum_in_reference_order(orc, mbavo, gpu_ctx, P, S):
    """Per-patch costs for patch sizes 2 .. 128 with an odd number of blur samples (residuals with full 53-bit
    mantissas, so the ORDER of the sum over a patch's pixels shows): power-of-two patches follow the stride-halving tree of
    the reference's shared-memory reduce() (reduction.h:13-55), the others the ascending sum (A10) -- equal to the
    oracle's bit for bit up to the rare fp32 weight flips."""
    sc = scenes.Scene(S=S, F=2, k=4, P=P, K=150, kp="random", seed=900 + P)
    p, keep = sc.oracle_problem(orc)
    ro = orc.evaluate(p)
    d = scenes.DeviceScene(sc)
    fb, pc, valid = scenes.gpu_eval_batch(gpu_ctx, [d], 4)
    assert es.rel(fb, ro["frame_blocks"]) < 1e-9
    want_pc = ro["patch_blocks"].reshape(-1, sc.E)[:, 0]
    got_pc = pc.ravel()[:want_pc.size]
    assert (got_pc != want_pc).sum() <= max(1, int(0.01 * want_pc.size)), int((got_pc != want_pc).sum())
    assert np.abs(got_pc - want_pc).max() <= 1e-5 * np.abs(want_pc).max()


def test_flat_tolerance_failure_rate_is_bounded(orc, mbavo, gpu_ctx):
    """The widened small-problem tolerance of es.tol() must not hide a NEW class of difference: with a FLAT 1e-9 on the
    packed blocks the known one-ulp fp32-weight flips fail about once in 2 000 random problems (profiles/r02_fuzz.txt:
    6 of 12 000).  200 further seeds: at most ONE may exceed the flat bound, and a failure must stay inside es.tol()."""
    worst = []
    for seed in range(5000, 5200):
        try:
            es.random_problem_matches_oracle(orc, gpu_ctx, seed, tol=lambda sc: 1e-9)
        except AssertionError:
            worst.append(seed)
    for seed in worst:  # whatever exceeded the flat bound is one of the small-problem flips: inside the stated tolerance
        es.random_problem_matches_oracle(orc, gpu_ctx, seed)
    assert len(worst) <= 1, worst
