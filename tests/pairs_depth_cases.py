"""Inputs of the depth-stage tests on option-laden objects and on the rounds object (helper, no test in it), made once on the host
so that tests/test_pairs_depth_options_inputs.py can assert without a GPU what tests/test_gpu_pairs_depth_options.py and
tests/test_gpu_pairs_depth_rounds.py rest on.

The option-laden objects are pairs_oracle.OBJECTS A - D, untouched.  The rounds object is one every-candidate object of 128 x 136
with L = 1 and the 8-pixel pattern, filled through prepare_points so that K is exact: capacity 17408, pair 0 with K = 16385 (65 tiles
of 256: workgroup 0 of the 256-keypoint kernels takes a second tile of one keypoint; 129 tiles of 128: workgroup 0 of the P = 8
kernels takes three), pair 1 with K = 17000 (workgroups 0 - 2 take a second tile of 256, the last ragged; workgroups 0 - 4 three tiles
of 128, the rest two)."""
import numpy as np

import pairs_carry_ref as cref
import pairs_cases
import pairs_oracle as po
import pairs_refine_ref as ref
from mba_vo_amd import synth

# ---- options of the calls, shared by the GPU files and the CPU preconditions
REFINE = dict(min_info=150.0)  # (on object B every keypoint is full and informed: a floor on h_rho leaves some in place on every object)
FILTER = dict(prior_rel_sigma=0.1, sigma_i=2.0, gate_chi2=9.0)
ND, ABSOLUTE, RELATIVE, MIN_RATIO = 6, (0.3, 1.1), (0.6, 1.5), 1.02
SMOOTH = dict(radius=3, min_support=2, max_rel_diff=0.1, strength=0.7, fill=1)
SMOOTH_OF = {"C": dict(SMOOTH, min_support=16, max_rel_diff=0.2)}  # (every candidate: a keypoint without two neighbours does not occur)
SAVE = dict(radius=2, deflate=0.8)
ADOPT = dict(min_support=2, max_rel_diff=0.1)
CARRY_PAIRS = {"B": [2], "D": [0, 2]}  # B: the pair with the second frame, on camera 1; D: two pairs on cameras 0 and 2
_Q = np.array([0.01, -0.02, 0.015, 1.0])
TILT = np.concatenate([[0.05, -0.03, 0.3], _Q / np.linalg.norm(_Q)])
CARRY_STEP = np.array([0.3, -0.2, 0.15])  # added to the new keyframe's position, so that some points leave the image


def smooth_opts(name):
    return SMOOTH_OF.get(name, SMOOTH)


def surface_depths(rng, n):
    """Two surfaces 40 % apart with 3 % of noise, and one keypoint in ten somewhere else."""
    z = np.where(rng.uniform(size=n) < 0.5, 2.0, 2.8) * (1.0 + rng.uniform(-0.03, 0.03, n))
    out = rng.uniform(size=n) < 0.1
    return np.where(out, rng.uniform(0.5, 6.0, n), z)


def harness_motion(nb, N):
    """The motion of the smoothing test: harness knots with a little noise, every sample on segment 0."""
    rng = np.random.default_rng(11)
    kt, kR = np.zeros((nb, N, 3)), np.zeros((nb, N, 4))
    for b in range(nb):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.02, 3)
    return dict(cap=(0.4 + 0.05 * np.arange(nb)) * 0.5, exp=np.full(nb, 0.04), t0=np.zeros(nb), dt=0.5, kt=kt, kR=kR)


# ---------------------------------------------------------------------------------------------------------------- objects A - D
def second_points(name):
    """The second keyframe's lists of a points object: the first one's lengths, other points."""
    o = po.OBJECTS[name]
    rng = np.random.default_rng(9100 + o["seed"])
    pts = []
    for n in o["lengths"]:
        xy = np.stack([rng.uniform(-2, o["W"] + 2, n), rng.uniform(-2, o["H"] + 2, n)], 1)
        xy[::3] = np.floor(xy[::3])
        pts.append((np.ascontiguousarray(xy), np.ascontiguousarray(rng.uniform(1.0, 3.0, n))))
    return pts


def second_inputs(name):
    """The composite inputs after the carry's update: object B's second frame (pairs_oracle.second_frame), object D's second lists
    under another motion."""
    if name == "B":
        return po.second_frame(name)
    c = dict(po.inputs(name))
    c.update(points=second_points(name), motion=po.motion(po.OBJECTS[name], seed=1))
    return c


def carry_pose(lib, capi, name, b):
    """T (7) of pair b's new keyframe in its old one's frame: pairs_carry_ref.relative_pose of the pair's mid-exposure poses under
    the object's first and second motion, the second moved by CARRY_STEP."""
    o, m0, m1 = po.OBJECTS[name], po.inputs(name)["motion"], second_inputs(name)["motion"]
    ends = []
    for m in (m0, m1):
        e = dict(S=o["S"], N=o["N"], cap=m["cap"][b:b + 1], exp=m["exp"][b:b + 1], t0=float(m["t0"][b]), dt=float(m["dt"]), kt=m["kt"][b].ravel(),
                 kR=m["kR"][b].ravel())
        p, q = ref.poses(lib, capi, e, o["k"])[o["S"] // 2]
        ends.append((p, q / np.linalg.norm(q)))
    return cref.relative_pose(ends[0][0], ends[0][1], ends[1][0] + CARRY_STEP, ends[1][1])


# ---------------------------------------------------------------------------------------------------------------- the rounds object
ROUNDS = dict(B=2, L=1, H=128, W=136, S=3, k=4, N=4, KS=(16385, 17000))
INVALID = (np.nan, np.inf, 0.0, -2.0, np.nan, np.inf)
_ROUNDS = {}


def invalid_at(K):
    return sorted({0, 255, 256, 16383, 16384, K - 1})


def rounds_lists(which=0):
    """Per pair (xy K x 2 whole pixels, z K): 95 % distinct pixels drawn over the image and 5 % of them again, so that about a tenth
    share a pixel; depths on two surfaces plus outliers, invalid ones at `invalid_at`.  which: 0 the keyframe, 1 the next one."""
    if which not in _ROUNDS:
        r = ROUNDS
        rng = np.random.default_rng(360 + which)
        out = []
        for K in r["KS"]:
            n = K - K // 20
            pix = rng.permutation(r["H"] * r["W"])[:n]
            pix = np.concatenate([pix, pix[rng.permutation(n)[:K - n]]])[rng.permutation(K)]
            xy = np.stack([pix % r["W"], pix // r["W"]], 1).astype(np.float64)
            z = surface_depths(rng, K)
            z[invalid_at(K)] = INVALID[:len(invalid_at(K))]
            out.append((np.ascontiguousarray(xy), z))
        _ROUNDS[which] = out
    return _ROUNDS[which]


def rounds_images():
    """(sharp, blur) 2 x 128 x 136 uint8."""
    sharp, _, blur = pairs_cases.inputs(ROUNDS["B"], ROUNDS["H"], ROUNDS["W"], special=False)
    return sharp, blur


def rounds_intr():
    return np.array([ROUNDS["W"] / 2.0, ROUNDS["W"] / 2.0, ROUNDS["W"] / 2.0, ROUNDS["H"] / 2.0])


def rounds_entries(which=0):
    """read_entry-shaped dicts of the two pairs from the host inputs alone (float gradients, the default intrinsics and Huber)."""
    r, m = ROUNDS, harness_motion(ROUNDS["B"], ROUNDS["N"])
    sharp, blur = rounds_images()
    out = []
    for b, (xy, z) in enumerate(rounds_lists(which)):
        out.append(dict(S=r["S"], F=1, K=len(z), P=8, k=r["k"], N=r["N"], H=r["H"], W=r["W"], fmt=0, ref=sharp[b], word_I=None,
                        grad=np.ascontiguousarray(synth.image_gradients(sharp[b])), curs=[blur[b]], xy=xy, z=z, stride=2,
                        pattern=np.ascontiguousarray(synth.PATTERN8, dtype=np.int32).ravel(), intr=rounds_intr(), cap=m["cap"][b:b + 1].copy(),
                        exp=m["exp"][b:b + 1].copy(), t0=float(m["t0"][b]), dt=float(m["dt"]), kt=m["kt"][b].ravel().copy(), kR=m["kR"][b].ravel().copy(),
                        start=np.array([0], np.int32), huber=10.0, outlier=None, num_bad=0))
    return out


def rounds_poses():
    """T (2 x 7) of the rounds carry: a tilt with a step forward, and a third of a pixel sideways at depth 2."""
    return np.stack([TILT, np.array([-2.0 / (3 * 68.0), 0, 0, 0, 0, 0, 1.0])])
