"""Shared by tests/test_pairs_hyp_api.py (CPU) and tests/test_gpu_pairs_hyp.py (GPU): mbavo_pairs_predict_hypotheses restated --
tangent, score, eligibility and winner in Python floats (IEEE doubles, no contraction), the candidate knots with the C ABI's own
host algebra (mbavo_se3_exp, mbavo_spline_transform_by_right) as tests/pairs_track.host_predict forms the predict's -- and the
inputs of the winner checks.

The winner inputs.  Per pair a keyframe that sees the textured plane z = D from the identity pose, a tracker state on a slow
harness spline with a stored velocity of about 0.3 m and 0.05 rad per frame, and a blurred current frame rendered ON THE KNOTS OF
ONE HYPOTHESIS, m* (TRUTH): the camera stopped, doubled its speed, reversed, took an extra rotation, halved its speed, or went on
as predicted (m* = 0).  The frames are rendered on the CPU with the oracle's restatement of the generator
(generate_synthetic_data.cpp:127-214: orc_warp_image, orc_synthesize_blur) -- the same images workloads.RenderedScene's device
renderer gives (tests/test_gpu_frontend.py holds the two renderers to each other) -- so that the CPU file can assert with the
oracle what the GPU file rests on: the scores are well separated, the flung-out hypothesis loses every pixel, the others keep most."""
import ctypes as C

import numpy as np

import frontend
import pairs_ref
import pairs_step as ps
from mba_vo_amd import synth

NONE_ELIGIBLE = 1
LEVELS, BORDER, S, P, HUBER, D = 3, 4, 8, 8, 10.0, 7.5
SCORE_REL = 1e-9  # what tests/test_gpu_pairs_oracle.py holds the cost to

# hypotheses 1 .. 7 of the winner checks: (scale, twist (v, w)); hypothesis 6 throws the scene out of the image
WIN_SCALES = (0.0, 2.0, -1.0, 1.0, 1.0, 1.0, 0.5)
WIN_TWISTS = (None, None, None, (0, 0, 0, 0, 0.06, 0), (0, 0, 0, -0.06, 0, 0), (1e4, 0, 0, 0, 0, 0), None)
FLUNG = 6
TRUTH = (1, 2, 0, 4, 3, 5, 7)  # m* of pair b
WIN_CASES = [(1, 120, 160, 2), (7, 120, 160, 4)]  # the smallest of pairs_step.ASSESS_CASES


def tangent(velocity, dt_frame, m, scale, twist):
    """tangent_m: 6 Python floats."""
    if m == 0:
        return [float(v) * dt_frame for v in velocity]
    return [(float(scale) * float(v)) * dt_frame + float(tw) for v, tw in zip(velocity, twist)]


def candidate(lib, dp, st, cap, m, scale=0.0, twist=(0.0,) * 6):
    """Candidate m of the state `st` (a VoState before the call) at capture time cap: (knots_t 3N, knots_R 4N)."""
    N = st.N
    kt, kR = np.array(st.knots_t[:3 * N]), np.array(st.knots_R[:4 * N])
    dt_frame = float(cap) - st.prev_timestamp
    tan, dT = np.array(tangent(list(st.velocity), dt_frame, m, scale, twist)), np.zeros(7)
    assert lib.mbavo_se3_exp(dp(tan), dp(dT)) == 0
    q, t = np.ascontiguousarray(dT[3:]), np.ascontiguousarray(dT[:3])
    assert lib.mbavo_spline_transform_by_right(dp(kt), dp(kR), N, dp(q), dp(t)) == 0
    return kt, kR


def candidates(lib, dp, st, cap, scales, twists):
    """All 1 + len(scales) candidates of one pair."""
    out = [candidate(lib, dp, st, cap, 0)]
    for m, (s, tw) in enumerate(zip(scales, twists), start=1):
        out.append(candidate(lib, dp, st, cap, m, s, (0.0,) * 6 if tw is None else tw))
    return out


def score(cost, K, Ppx, valid):
    KP = float(K) * float(Ppx)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((np.float64(cost) * np.float64(KP)) / np.float64(valid))


def eligible(sc, K, Ppx, valid, min_valid_frac):
    f = 0.5 if min_valid_frac == 0 else float(min_valid_frac)
    return bool(K > 0 and valid >= f * (float(K) * float(Ppx)) and np.isfinite(sc))


def winner(scores, elig, min_gain=0.0):
    """(winner, status, number eligible)."""
    c = None
    for m in range(1, len(scores)):
        if elig[m] and (c is None or scores[m] < scores[c]):
            c = m
    w = 0
    if c is not None and (not elig[0] or scores[c] < scores[0] * (1.0 - float(min_gain))):
        w = c
    n = int(sum(bool(e) for e in elig))
    return w, (NONE_ELIGIBLE if n == 0 else 0), n


def oracle_scores(orc, entry, cands, min_valid_frac=0.0):
    """The oracle on one read_entry-shaped entry with each candidate's knots in turn: (scores, valid counts, eligible, costs)."""
    import pairs_oracle as po
    scores, valids, elig, costs = [], [], [], []
    for kt, kR in cands:
        e = dict(entry, kt=np.ascontiguousarray(kt, dtype=np.float64).ravel().copy(), kR=np.ascontiguousarray(kR, dtype=np.float64).ravel().copy(),
                 outlier=None, num_bad=0)
        p, keep = po.problem_of(orc, e)
        if e["K"] > 0:
            cost = float(orc.evaluate(p, with_hessian=False)["frame_blocks"][0, 0])
            valid = float(orc.count_valid(p)[0])
        else:
            cost, valid = 0.0, 0.0
        sc = score(cost, e["K"], e["P"], valid)
        scores.append(sc); valids.append(valid); costs.append(cost)
        elig.append(eligible(sc, e["K"], e["P"], valid, min_valid_frac))
    return scores, valids, elig, costs


# ---------------------------------------------------------------------------------------------------------------- the winner inputs
_CASES = {}


def win_states(capi, B, k):
    """The B states the winner inputs are rendered from (no oracle, no device)."""
    rng = np.random.default_rng(4200 + 10 * B + k)
    cap = 0.55 + 0.013 * np.arange(B)
    states = (capi.VoState * B)()
    for b, st in enumerate(states):
        kt, kR = synth.trajectory("harness", ps.N_KNOTS, 0.004, 0.005)
        st.t0, st.dt, st.N, st.is_first = 0.0, 0.5, ps.N_KNOTS, 0
        st.knots_t[:3 * ps.N_KNOTS] = kt.ravel().tolist()
        st.knots_R[:4 * ps.N_KNOTS] = kR.ravel().tolist()
        q = rng.normal(0, 1, 4)
        st.T_keyframe[:] = np.r_[rng.normal(0, 1, 3), q / np.linalg.norm(q)].tolist()
        st.T_prev_b2w[:] = [0.0, 0, 0, 0, 0, 0, 1]
        v, w = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
        v[2] *= 0.3  # (mostly across the image: motion along the axis barely moves a pixel)
        w[2] *= 0.3
        vel = np.r_[3.0 * v / np.linalg.norm(v), 0.5 * w / np.linalg.norm(w)]
        st.velocity[:] = vel.tolist()
        st.prev_timestamp = float(cap[b]) - 0.1
    return states, cap, np.full(B, 0.04)


def win_case(orc, mbavo, B, H, W, k):
    """dict(B, H, W, k, sharp, depth, blur [B x H x W], states, cap, exp, truth, cands [b][m] (kt, kR), intr), made once."""
    key = (B, H, W, k)
    if key in _CASES:
        return _CASES[key]
    lib, capi = mbavo.load(), mbavo.capi
    L = orc.lib()
    states, cap, exp = win_states(capi, B, k)
    intr = np.array([W / 2.0, W / 2.0, W / 2.0, H / 2.0])
    ident_q, ident_t = np.array([0.0, 0, 0, 1]), np.zeros(3)
    sharp, depth, blur, cands = [], [], [], []
    for b in range(B):
        I0 = synth.texture_image(H, W, seed=31 + b, octaves=(32, 16, 8, 4))
        img = np.zeros((H, W), np.uint8)
        L.orc_warp_image(orc.u8p(I0), H, W, orc.dp(ident_q), orc.dp(ident_t), float(D), orc.dp(intr), orc.u8p(img))
        sharp.append(img)
        depth.append(frontend.plane_depth_map(H, W, intr, ident_q, ident_t, D))
        cs = candidates(lib, capi.dp, states[b], cap[b], WIN_SCALES, WIN_TWISTS)
        kt, kR = (np.ascontiguousarray(a) for a in cs[TRUTH[b]])
        out = np.zeros((H, W), np.uint8)
        # (the frame's spline starts at cap - exp / 2, as the predict publishes it: blur_aware_direct_tracker.cpp:131)
        L.orc_synthesize_blur(orc.u8p(I0), H, W, float(D), orc.dp(intr), k, float(cap[b] - 0.5 * exp[b]), 0.5, orc.dp(kt), orc.dp(kR),
                              float(cap[b]), float(exp[b]), 8, orc.u8p(out))
        blur.append(out)
        cands.append(cs)
    case = dict(B=B, H=H, W=W, k=k, sharp=np.ascontiguousarray(np.stack(sharp)), depth=np.ascontiguousarray(np.stack(depth)),
                blur=np.ascontiguousarray(np.stack(blur)), states=states, cap=cap, exp=exp, truth=TRUTH[:B], cands=cands, intr=intr)
    _CASES[key] = case
    return case


# the eligibility check: min_valid_frac = 1 with pair FAST four times as fast (every hypothesis loses a pixel) and pair BLANK on a
# blank keyframe (no keypoint); hypothesis 3 is the flung-out one
ELIG_SCALES, ELIG_TWISTS, ELIG_FLUNG, FAST, BLANK = (1.5, 2.0, 1.0), (None, None, WIN_TWISTS[FLUNG - 1]), 3, 2, 4


def elig_case(orc, mbavo):
    """(case, states) of the eligibility check, from the second winner case."""
    capi = mbavo.capi
    base = win_case(orc, mbavo, *WIN_CASES[1])
    case = dict(base, sharp=base["sharp"].copy())
    case["sharp"][BLANK] = 128
    states = (capi.VoState * base["B"])()
    for b in range(base["B"]):
        C.memmove(C.byref(states[b]), C.byref(base["states"][b]), C.sizeof(states[b]))
    for j in range(6):
        states[FAST].velocity[j] *= 4.0
    case["states"] = states
    case["cands"] = [candidates(mbavo.load(), capi.dp, states[b], case["cap"][b], ELIG_SCALES, ELIG_TWISTS) for b in range(base["B"])]
    return case, states


def host_entry(case, b, level, cell=ps.CELL, thr=ps.THR):
    """The read_entry-shaped dict of pair b's level-`level` entry after the call, from the numpy restatements alone (the knots are
    left to the caller)."""
    H, W = case["H"], case["W"]
    refs, curs = synth.pyramid(np.ascontiguousarray(case["sharp"][b]), LEVELS), synth.pyramid(np.ascontiguousarray(case["blur"][b]), LEVELS)
    Hl, Wl = H >> level, W >> level
    xy, z = pairs_ref.keypoints(refs[level], level, H, W, cell, cell, thr, case["depth"][b], BORDER)
    cap, exp = float(case["cap"][b]), float(case["exp"][b])
    t0 = cap - 0.5 * exp
    return dict(S=S, F=1, K=len(z), P=P, k=case["k"], N=ps.N_KNOTS, H=Hl, W=Wl, fmt=0, ref=refs[level], word_I=None,
                grad=np.ascontiguousarray(synth.image_gradients(refs[level])), curs=[curs[level]],
                xy=np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2), z=np.ascontiguousarray(z, dtype=np.float64), stride=2,
                pattern=np.ascontiguousarray(synth.PATTERN8, dtype=np.int32), intr=np.array([v / float(1 << level) for v in case["intr"]]),
                cap=np.array([cap]), exp=np.array([exp]), t0=t0, dt=0.5, kt=None, kR=None,
                start=np.array([synth.segment_start_index(cap, t0, 0.5)], np.int32), huber=HUBER, outlier=None, num_bad=0)
