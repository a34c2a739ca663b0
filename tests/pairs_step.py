"""Shared by tests/test_pairs_step_api.py (CPU) and tests/test_gpu_pairs_step.py (GPU): the inputs of the mbavo_pairs_assess /
mbavo_pairs_update checks, the oracle's answers to them, and the bounds.  Everything here runs without a GPU, so the CPU file can
assert that the GPU file's inputs are good ones: both verdicts occur and no average lies near a threshold."""
import ctypes as C

import numpy as np

import frontend
import pairs_ref
from mba_vo_amd import synth

FLOW0, FLOW1, KERNEL = frontend.DEFAULTS["flow0"], frontend.DEFAULTS["flow1"], frontend.DEFAULTS["kernel"]
CELL, THR = 10, 3.0
REL = 2.0 ** -23  # one float ulp: (float) of a double sum good to far below 2^-24, then a correctly rounded monotonic sqrtf
# Absolute floor for averages near zero motion, where the sum is rounding noise of the "+ 1e-8" projection: 4 x the largest
# difference between the oracle and its own FMA build (libmbavo_oracle_fma.so) over the identity-motion versions of ASSESS_CASES,
# measured with identity_motion_noise() below: 0.0 for avg_flow and for avg_kernel -- the two builds return the same floats on every
# pair (the averages there are ~1e-6 px, the bias of the "+ 1e-8" itself; contraction moves the double sums far below a float ulp).
# So the floor is zero and the bound is the relative one alone.  tests/test_pairs_step_api.py re-measures it wherever the FMA
# build exists.
MEASURED_FMA_NOISE = 0.0
FLOOR = 4.0 * MEASURED_FMA_NOISE

# (B, H, W, spline degree): the issue's sizes; the degree alternates so that both spline forms are sampled on the device
ASSESS_CASES = [(1, 120, 160, 2), (7, 120, 160, 4), (64, 120, 160, 2), (1, 240, 320, 4), (7, 240, 320, 2), (64, 240, 320, 4)]
N_KNOTS = 6
# motion scale of pair b = SCALES[b % len]: from nearly at rest to far past both flow thresholds
SCALES = (0.02, 0.35, 0.6, 1.1, 1.5, 2.6, 0.1, 1.9, 3.4)


def bound(want):
    return REL * abs(want) + FLOOR


def assess_inputs(B, H, W, k, seed=None, identity=False):
    """Images, depth maps and motion of one assess case: dict(sharp, depth, blur [B x H x W], cap, exp, t0 [B], dt, kt [B x N x 3],
    kR [B x N x 4], intr).  Motion: synth.trajectory("harness") scaled per pair; identity: every knot the identity."""
    seed = B + H if seed is None else seed
    rng = np.random.default_rng(seed)
    base = synth.texture_image(H, W, seed=seed, octaves=(32, 16, 8, 4))
    other = synth.texture_image(H, W, seed=seed + 100, octaves=(32, 16, 8, 4))
    sharp = np.ascontiguousarray(np.stack([np.roll(base, (7 * b, 13 * b), (0, 1)) for b in range(B)]))
    blur = np.ascontiguousarray(np.stack([np.roll(other, (3 * b + 1, 5 * b + 2), (0, 1)) for b in range(B)]))
    depth = rng.uniform(1.0, 3.0, (B, H, W)).astype(np.float32)
    depth[rng.uniform(0, 1, (B, H, W)) < 0.1] = 0.0
    kt, kR = np.zeros((B, N_KNOTS, 3)), np.zeros((B, N_KNOTS, 4))
    for b in range(B):
        s = SCALES[b % len(SCALES)]
        kt[b], kR[b] = synth.trajectory("harness", N_KNOTS, 0.012 * s, 0.02 * s)
        if identity:
            kt[b], kR[b] = 0.0, np.array([0.0, 0, 0, 1])
    cap = 0.55 + 0.013 * (np.arange(B) % 11)
    exp = np.where(np.arange(B) % 4 == 3, 0.45, 0.04)  # (a long exposure on every fourth pair: the blur-kernel test decides there)
    return dict(B=B, H=H, W=W, k=k, sharp=sharp, depth=depth, blur=blur, cap=cap, exp=exp, t0=np.zeros(B), dt=0.5,
                kt=kt, kR=kR, intr=np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0]))


def host_keypoints0(case, border):
    """Level-0 keypoints of every pair by the numpy restatement (tests/pairs_ref.py: bit for bit what the device prepares)."""
    return [pairs_ref.keypoints(case["sharp"][b], 0, case["H"], case["W"], CELL, CELL, THR, case["depth"][b], border)
            for b in range(case["B"])]


def oracle_assess(orc, intr, xy, z, k, t0, dt, kt, kR, cap, exp, thresholds=(FLOW0, FLOW1, KERNEL)):
    """orc_is_keyframe (oracle/mbavo_oracle_vo.c:255) on one pair: (verdict, avg_flow, avg_kernel)."""
    xy, z = np.ascontiguousarray(xy, dtype=np.float64).ravel(), np.ascontiguousarray(z, dtype=np.float64)
    kt, kR = np.ascontiguousarray(kt, dtype=np.float64).ravel(), np.ascontiguousarray(kR, dtype=np.float64).ravel()
    intr = np.ascontiguousarray(intr, dtype=np.float64)
    af, ak = np.zeros(1), np.zeros(1)
    v = orc.lib().orc_is_keyframe(orc.dp(intr), orc.dp(xy), orc.dp(z), int(z.size), int(k), float(t0), float(dt), orc.dp(kt), orc.dp(kR),
                                  float(cap), float(exp), float(thresholds[0]), float(thresholds[1]), float(thresholds[2]), orc.dp(af), orc.dp(ak))
    return int(v), float(af[0]), float(ak[0])


def margin_ok(af, ak, extra=0.0, thresholds=(FLOW0, FLOW1, KERNEL)):
    """The averages lie further than the bound (plus `extra`) from every threshold they are compared with."""
    return (abs(af - thresholds[0]) > bound(af) + extra and abs(af - thresholds[1]) > bound(af) + extra
            and abs(ak - thresholds[2]) > bound(ak) + extra)


def count_behind(intr, xy, z, poses):
    """numpy count of the projections with Pc.z < 0: keypoints x the given poses (t[3], q xyzw; body to world)."""
    fx, fy, cx, cy = intr
    P = np.stack([(xy[:, 0] - cx) / fx * z, (xy[:, 1] - cy) / fy * z, z], 1)
    n = 0
    for T in poses:
        R = frontend._quat_R(np.asarray(T[3:]) / np.linalg.norm(T[3:]))
        n += int((((P - np.asarray(T[:3])) @ R)[:, 2] < 0).sum())
    return n


def identity_motion_noise(orc, fma):
    """max |oracle - FMA build| of avg_flow and avg_kernel over the identity-motion versions of ASSESS_CASES."""
    worst = [0.0, 0.0]
    for (B, H, W, k) in ASSESS_CASES:
        case = assess_inputs(B, H, W, k, identity=True)
        for b, (xy, z) in enumerate(host_keypoints0(case, 4)):
            a = oracle_assess(orc, case["intr"], xy, z, k, 0.0, 0.5, case["kt"][b], case["kR"][b], case["cap"][b], case["exp"][b])
            f = oracle_assess(fma, case["intr"], xy, z, k, 0.0, 0.5, case["kt"][b], case["kR"][b], case["cap"][b], case["exp"][b])
            worst = [max(worst[0], abs(a[1] - f[1])), max(worst[1], abs(a[2] - f[2]))]
    return worst


# ---- the teacher-forced batch (check 7)
SEQ_SEEDS = (3, 4, 5, 7, 9, 10)
SEQ_M = 8
# the pixel change a 1e-4 knot difference allows: the knot tolerance of tests/test_gpu_lm_batch_levels._check_against times the
# focal length
KNOT_TOL = 1e-4


def knot_pixel_bound(intr):
    return KNOT_TOL * float(intr[0])


def predict(lib, dp, st, cap, exp):
    """The constant-velocity prediction of trackFrame (.cpp:119-141) from a tracker state before the frame: (t0, kt, kR, dt_frame)
    with the C ABI's own pose algebra: mbavo_se3_exp and mbavo_spline_transform_by_right."""
    N = st.N
    kt, kR = np.array(st.knots_t[:3 * N]), np.array(st.knots_R[:4 * N])
    dt_frame = cap - st.prev_timestamp
    vel = np.array([v * dt_frame for v in st.velocity])
    dT = np.zeros(7)
    assert lib.mbavo_se3_exp(dp(vel), dp(dT)) == 0
    q, t = np.ascontiguousarray(dT[3:]), np.ascontiguousarray(dT[:3])
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), N, dp(q), dp(t)) == 0
    return cap - 0.5 * exp, kt, kR, dt_frame
