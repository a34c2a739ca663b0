"""CPU-only side of tests/test_gpu_lm_batch_dense.py: the dense (P = 1, K in the thousands) scenes the batched LM is held to
the host loop and the oracle on, and the rule their seeds are chosen by.

k_lm_decide (mba-vo_amd/csrc/lm_batch.hip) has two forms of detectOutliersAndUploadToGpu, split at K = 512 (64 lanes x 8 patch
costs in registers, or three strided passes over global memory); the scenes here put K on both sides of that within one batch
(levels), right at it (cuts: K = 511, 512, 513, 577), and give it patch costs of exactly 0 (flat): the statistics skip costs
below 1e-8, the flagging pass does not -- and on the offset variants of the flat scenes it has to flag them.

The discrete record sequence (level, iteration, kind, outlier count) is asserted exactly on the GPU, so a case must not sit
where rounding decides.  seed_ok() is that condition, from the oracle alone: the pinned build (-ffp-contract=off) and its
contracted twin (oracle.binding.fma_variant()) give the same sequence, and in the pinned run every accept test keeps
|quality - min_q| > 1e-6 and |eval - cand| > 1e-9 eval, every outlier test | |c - mu| - bound | > 1e-6 bound.  The seeds
below were chosen with first_ok_seed(); tests/test_lm_dense_seeds.py re-checks them without a GPU."""
import numpy as np

import tracking

SOLVE = dict(tracking.OPTS)
SOLVE12 = dict(tracking.OPTS, max_num_iterations=12)  # the cuts and the flat scenes (as test_lm_batch_pose_entries_same_bits)

# --- 1. B = 4 pairs, two levels: 48 x 64 (K = 960 | 240) and 96 x 128 (K = 7488 | 1872), F = 1 and 2 -------------------------
LEVEL_SHAPES = ((48, 64, 1), (96, 128, 1), (48, 64, 2), (96, 128, 2))  # (H, W, F) of pair b
LEVEL_CASES = ((4, 0, 0.0), (2, 0, 0.0), (4, 1, -1.0))                   # (k, solver, fast_solve_ratio)
# seeds of pair b for (k, solver): 2026-10-18, first_ok_seed() from 300 + 100 * case + 10 * b
LEVEL_SEEDS = {(4, 0): (300, 310, 320, 330), (2, 0): (400, 410, 420, 430), (4, 1): (500, 510, 520, 530)}

# --- 2. one dense one-level 48 x 64 scene (K = 960) cut to the first K keypoints -------------------------------------------
CUT_K = (511, 512, 513, 577)  # below, at and above 64 x 8; 577 = 9 x 64 + 1: a last strided round of one lane
CUT_SEED = 501                # 2026-10-18, first_ok_seed() from 500: all four cuts pass and accept a step with outliers

# --- 3. exact-zero patch costs: a flat rectangle in keyframe and current image ---------------------------------------------
FLAT_H, FLAT_W = 48, 64
FLAT_RECT = (16, 32, 18, 46)  # rows [16, 32), columns [18, 46)
FLAT_EDGE = 2                 # the current image is the keyframe's level this far inside the rectangle
FLAT_INNER = 4                # keypoints this far inside see only those pixels (the motion is below 2 pixels)
FLAT_LEVEL = 0                # see flat_scene()
# variant: (keypoints inside this border, every n-th of them, contrast divisor of the texture, +-noise and brightness added to the
# current image outside the rectangle, make_tracking_scene's perturb).  16 x 32 = 512, 24 x 40 = 960, every second of 960 = 480.
FLAT = {"K512": (16, 1, 1, 3, 0, 4e-3), "K960": (12, 1, 1, 3, 0, 4e-3),
        "K480_offset": (12, 2, 2, 1, 40, 1e-3), "K960_offset": (12, 1, 2, 1, 40, 1e-3)}
# 2026-10-18, the first seed from 600 / 700 / 800 / 800 that passes seed_ok() and flat_costs_ok() and has an accepted step with
# outliers; the offset variants: with flags_the_zero_costs()
FLAT_SEEDS = {"K512": 607, "K960": 701, "K480_offset": 804, "K960_offset": 801}


def level_scenes(orc, k, seeds):
    return [tracking.make_tracking_scene(orc, H=H, W=W, levels=2, S=4, k=k, F=F, seed=s, mode="dense")
            for (H, W, F), s in zip(LEVEL_SHAPES, seeds)]


def cut_scene(full, K):
    """The one-level scene `full` with the first K keypoints of its list."""
    lv = full["levels"][0]
    assert len(full["levels"]) == 1 and lv["kp_xy"].shape[0] >= K
    cut = dict(lv, kp_xy=np.ascontiguousarray(lv["kp_xy"][:K]), kp_z=np.ascontiguousarray(lv["kp_z"][:K]))
    return dict(full, levels=[cut])


def cut_scenes(orc, seed, k=4):
    full = tracking.make_tracking_scene(orc, H=48, W=64, levels=1, S=4, k=k, F=1, seed=seed, mode="dense")
    assert full["levels"][0]["kp_xy"].shape[0] >= 600
    return [cut_scene(full, K) for K in CUT_K]


def flat_scene(orc, variant, seed, k=4):
    """One dense pair (tracking.make_tracking_scene: 48 x 64, one level, F = 1, S = 4) whose keyframe has the rectangle FLAT_RECT
    painted in one grey level before the current image is warped from it along the ground-truth spline.  The current image
    then gets noise, and its pixels FLAT_EDGE or more inside the rectangle are set to the keyframe's level again: there the two
    images are equal, further than the motion from anything else.  The variants are the rows of FLAT.  K512 keeps the keypoints
    16 pixels from the border: 357 of its 512 patch costs are exact zeros, so its statistics rest on the 155 keypoints along
    the rectangle's edges; K960 has 354 zeros of 960.

    The two offset variants are there for the THIRD statistics pass, which compares the zero costs with the bound although the
    first two skip them.  On the plain variants 3 sigma is far above the mean, so no zero cost is ever flagged and that pass could
    skip them unnoticed.  With a texture of half the contrast and the current image 40 levels brighter outside the rectangle,
    every other residual is about 40 and the costs lie close together (3 sigma < mean): the oracle's first accepted step flags
    every zero cost (329 outliers for 288 zeros at K = 960; 158 for 144 at K = 480, every second keypoint of the same list).

    The level is 0: the oracle and the kernels interpolate with float weights w00 = 1 - dx - dy + dx dy, ..., whose rounded sum
    is not exactly 1, so four equal taps of value g come back as g only up to a float ulp -- a patch cost of 1e-12, not 0.
    Products with 0 are exact in every rounding and every contraction; with S samples of 0 against a pixel of 0 the residual,
    and the patch cost, is exactly 0.0."""
    y0, y1, x0, x1 = FLAT_RECT

    margin, stride, contrast, noise, offset, perturb = FLAT[variant]

    def paint(img):
        if contrast > 1:
            img[:] = 100 + img // contrast
        img[y0:y1, x0:x1] = FLAT_LEVEL

    sc = tracking.make_tracking_scene(orc, H=FLAT_H, W=FLAT_W, levels=1, S=4, k=k, F=1, seed=seed, mode="dense", paint=paint,
                                      perturb=perturb)
    rng = np.random.default_rng(seed + 7)
    lv = sc["levels"][0]
    cur = lv["cur"][0].astype(np.int32) + rng.integers(-noise, noise + 1, lv["cur"][0].shape) + offset
    cur = np.clip(cur, 0, 255).astype(np.uint8)
    e = FLAT_EDGE
    cur[y0 + e:y1 - e, x0 + e:x1 - e] = FLAT_LEVEL
    m = margin
    x, y = lv["kp_xy"].T
    keep = (x >= m) & (x < FLAT_W - m) & (y >= m) & (y < FLAT_H - m)
    sc["levels"] = [dict(lv, cur=[np.ascontiguousarray(cur)], kp_xy=np.ascontiguousarray(lv["kp_xy"][keep][::stride]),
                         kp_z=np.ascontiguousarray(lv["kp_z"][keep][::stride]))]
    return sc


def flat_inside(sc):
    """Which keypoints of a flat scene lie FLAT_INNER pixels or more inside the rectangle."""
    y0, y1, x0, x1 = FLAT_RECT
    x, y = sc["levels"][0]["kp_xy"].T
    m = FLAT_INNER
    return (x >= x0 + m) & (x < x1 - m) & (y >= y0 + m) & (y < y1 - m)


def initial_patch_costs(orc, sc):
    """The oracle's per-patch costs of frame 0 at the initial knots (level 0, no outlier flagged yet)."""
    lv = sc["levels"][0]
    K = lv["kp_xy"].shape[0]
    start = np.array([int((c - sc["t0"]) / sc["dt"]) for c in sc["cap"]], np.int32)
    kt, kR = sc["kt0"].ravel().copy(), sc["kR0"].ravel().copy()
    prob, keep = orc.make_problem(lv["S"], sc["F"], K, 1, sc["k"], sc["N"], lv["H"], lv["W"], lv["ref"], lv["grad"], lv["cur"],
                                  lv["kp_xy"], lv["kp_z"], lv["pattern"], sc["intr"], sc["cap"], sc["exp"], sc["t0"], sc["dt"],
                                  kt, kR, start, SOLVE["huber_k"])
    return orc.evaluate(prob)["patch_blocks"][0, :, 0].copy()


# --- the seed rule ---------------------------------------------------------------------------------------------------------
def sequence(trace):
    return [r[:4] for r in trace]


def accept_margins(trace, min_q):
    """Smallest |quality - min_q| and |eval - cand| / eval over the accept tests of a record list.  `eval` is the cost the
    candidate was compared with: the previous record's (an accepted step's own record already carries the re-evaluated cost)."""
    dq, dc = np.inf, np.inf
    for prev, r in zip(trace, trace[1:]):
        if r[2] in (1, 2):
            assert prev[0] == r[0]  # (a level begins with its kind-0 record)
            dq = min(dq, abs(r[8] - min_q))
            dc = min(dc, abs(prev[5] - r[6]) / prev[5] if prev[5] > 0 else 0.0)
    return dq, dc


def run_with_margin(orc, sc, opts):
    """tracking.run_oracle_tracker and the closest any outlier test of the run came to its bound (relative; orc_margins_*)."""
    L = orc.lib()
    L.orc_margins_reset()
    out = tracking.run_oracle_tracker(orc, sc, opts)
    mg = np.zeros(2)
    L.orc_margins_get(orc.dp(mg))
    return out, float(mg[1])


def seed_ok(orc, fma, sc, opts):
    """(ok, why, pinned run): the rule of this module's docstring for one scene."""
    a, outlier_margin = run_with_margin(orc, sc, opts)
    b = tracking.run_oracle_tracker(fma, sc, opts)
    if sequence(a["trace"]) != sequence(b["trace"]):
        return False, "pinned and contracted oracle part", a
    dq, dc = accept_margins(a["trace"], opts["min_step_quality"])
    if not (dq > 1e-6 and dc > 1e-9):
        return False, "accept test within its margin: |q - min_q| %.3e, |eval - cand| / eval %.3e" % (dq, dc), a
    if any(r[2] == 1 for r in a["trace"]) and not outlier_margin > 1e-6:
        return False, "outlier test within 1e-6 of its bound: %.3e" % outlier_margin, a
    return True, "", a


def first_ok_seed(orc, fma, make, opts, start, tries=40, also=lambda sc, run: True):
    """The first seed from `start` whose scene(s) `make(seed)` (a scene or a list of scenes) all pass seed_ok and `also`."""
    for seed in range(start, start + tries):
        scs = make(seed)
        scs = scs if isinstance(scs, list) else [scs]
        if all(ok and also(sc, run) for sc in scs for ok, _, run in [seed_ok(orc, fma, sc, opts)]):
            return seed
    raise RuntimeError("no seed in [%d, %d) passes" % (start, start + tries))


# --- what a run has to show for the test to mean something -------------------------------------------------------------------
def flags_large_K(trace, K0):
    """An accepted level-0 step with outliers flagged, the level's K above 512."""
    return K0 > 512 and any(r[0] == 0 and r[2] == 1 and r[3] > 0 for r in trace)


def outliers_change(trace):
    """The outlier count differs between two accepted steps of level 0."""
    return len({r[3] for r in trace if r[0] == 0 and r[2] == 1}) > 1


def flat_costs_ok(costs, inside):
    """At least 64 patch costs exactly 0.0, every keypoint well inside the rectangle among them, and every other cost above the
    1e-8 the statistics skip."""
    zero = costs == 0.0
    return int(zero.sum()) >= 64 and bool(np.all(costs[~zero] > 1e-8)) and int(inside.sum()) >= 64 and bool(np.all(zero[inside]))


def flags_the_zero_costs(trace, costs):
    """An accepted step whose outlier count is at least the number of exact-zero patch costs: they lay beyond the bound."""
    return any(r[2] == 1 and r[3] >= int((costs == 0.0).sum()) for r in trace)
