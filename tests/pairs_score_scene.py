"""The scene of the conditioning property of mbavo_pairs_set_detector (helper, no test in it): a deterministic synthetic keyframe
of vertical stripes with a sparse set of blobs over a depth plane, generated from a seed, and the condition number of the
translational (v_x, v_y) block of the report's info_unit on it.

Stripes are straight edges: they constrain v_x and say nothing about v_y.  The gradient magnitude picks the strongest pixel of
every cell, which is a stripe edge wherever the stripes' contrast exceeds the blobs'; the corner score picks blob corners alone.
So under the gradient magnitude the block's v_y entry rests on the few cells whose pick happens to touch a blob, and the block is
badly conditioned; under the score both entries rest on the same corners.

`entry` builds level 0 of one pair in the shape of pairs_oracle.read_entry from the restated selection (tests/pairs_score_ref.py),
`cpu_condition` evaluates it with the oracle and takes the block through the report restatement (tests/pairs_report_ref.py), as
tests/test_pairs_report_api.py does."""
import numpy as np

import pairs_oracle as po
import pairs_report_ref as rr
import pairs_score_ref as sr
from mba_vo_amd import synth

H, W, L, CELL, BORDER = 96, 128, 1, 8, 4
S, K_DEG, N, P = 3, 2, 2, 8
INTR = (W / 2.0, W / 2.0, W / 2.0, H / 2.0)
DEPTH = 2.0
RADIUS = 2
THR_GRAD, THR_SCORE = 4.0, 2.0
# the setting (see profiles/r45_pairs_score.txt for what was measured): grey levels of the stripes, their period, the blobs' step
# and how many of them
SETTING = dict(lo=70, hi=170, period=8, blob=40, n_blobs=12, seed=45)
# measured on the CPU with the oracle (tests/test_pairs_score_property_inputs.py asserts them): the block's condition number under
# the gradient magnitude and under the corner score, and their ratio
COND_GRAD, COND_SCORE = 46.43, 7.535
FACTOR = COND_GRAD / COND_SCORE  # 6.16


def keyframe(setting=SETTING):
    """The H x W keyframe: vertical stripes of `period` pixels between lo and hi, n_blobs squares of 5 x 5 pixels `blob` grey
    levels above what lies under them, at seeded positions."""
    s = setting
    x = np.mgrid[0:H, 0:W][1]
    img = np.where((x // (s["period"] // 2)) % 2 == 0, s["lo"], s["hi"]).astype(np.int32)
    rng = np.random.default_rng(s["seed"])
    for _ in range(s["n_blobs"]):
        y0, x0 = int(rng.integers(BORDER + 2, H - BORDER - 7)), int(rng.integers(BORDER + 2, W - BORDER - 7))
        img[y0:y0 + 5, x0:x0 + 5] += s["blob"]
    return np.clip(img, 0, 255).astype(np.uint8)


def inputs(setting=SETTING):
    """(sharp, depth, blur) of the one pair, 1 x H x W each: a depth plane, the current frame the keyframe a pixel to the right."""
    sharp = keyframe(setting)
    return sharp[None].copy(), np.full((1, H, W), DEPTH, np.float32), np.ascontiguousarray(np.roll(sharp, 1, 1))[None].copy()


def motion():
    """Identity knots around the capture time: the block is read at the pose the frames were made for."""
    kt, kR = np.zeros((1, N, 3)), np.zeros((1, N, 4))
    kR[..., 3] = 1.0
    return dict(cap=np.array([0.2]), exp=np.array([0.04]), t0=np.zeros(1), dt=0.5, kt=kt, kR=kR)


def entry(r, setting=SETTING):
    """Level 0 of the pair as pairs_oracle.read_entry would read it, keypoints from the restated selection under the corner score
    of radius r (0: under the gradient magnitude)."""
    sharp, depth, blur = inputs(setting)
    m = motion()
    xy, z = sr.keypoints(sharp[0], 0, H, W, CELL, THR_SCORE if r else THR_GRAD, depth[0], BORDER, r, dense=False)
    return dict(S=S, F=1, K=len(z), P=P, k=K_DEG, N=N, H=H, W=W, fmt=0, ref=sharp[0], word_I=None,
                grad=np.ascontiguousarray(synth.image_gradients(sharp[0])), curs=[blur[0]], xy=np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2),
                z=np.ascontiguousarray(z, dtype=np.float64), stride=2, pattern=np.ascontiguousarray(synth.PATTERN8, dtype=np.int32),
                intr=np.array(INTR, np.float64), cap=m["cap"].copy(), exp=m["exp"].copy(), t0=0.0, dt=float(m["dt"]), kt=m["kt"][0].ravel().copy(),
                kR=m["kR"][0].ravel().copy(), start=np.array([synth.segment_start_index(m["cap"][0], 0.0, m["dt"])], np.int32), huber=po.HUBER,
                outlier=None, num_bad=0)


def condition(info):
    """The condition number of the (v_x, v_y) block of a 6 x 6 info_unit: largest over smallest eigenvalue of the symmetric 2 x 2."""
    b = np.asarray(info, np.float64).reshape(6, 6)[:2, :2]
    w = np.linalg.eigvalsh(0.5 * (b + b.T))
    return float(w[1] / w[0]) if w[0] > 0 else float("inf")


def cpu_condition(orc, r, setting=SETTING):
    """(condition number, K, the 2 x 2 block) of the oracle's level-0 Hessian under the report restatement."""
    e = entry(r, setting)
    p, keep = po.problem_of(orc, e)
    _, _, Hl = rr.unpack(orc.evaluate(p)["frame_blocks"][0], K_DEG)
    s = int(e["start"][0])
    A = rr.shift_matrix(e["kt"].reshape(-1, 3)[s:s + K_DEG], e["kR"].reshape(-1, 4)[s:s + K_DEG])
    info = rr.info_unit(Hl, A, e["K"], P)
    return condition(info), e["K"], info[:2, :2].copy()
