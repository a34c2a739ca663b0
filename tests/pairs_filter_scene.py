"""Further blurred frames of the keyframes of tests/pairs_refine_scene.py for the depth-filter tests (helper, no test in it).

pairs_refine_scene keeps ONE rendered blurred frame per pair and exposes no renderer, so the frames here were rendered once on an
MI355X from its public pieces -- workloads.RenderedScene(3 pairs, 64 x 48, seed 30, plane at z = 2, frames 0.1 apart, exposure
0.04: the scene whose keyframes, blurred frames and knots are bit for bit those of tests/golden/refine_scene.npz) and
mbavo_synthesize_blur at 8 samples -- and are kept in tests/golden/filter_scene.npz: per pair T_MAX = 8 frames of the SAME keyframe
at capture times from the golden frame's (frame 0 IS the golden blurred frame) to 0.97 in equal steps, all inside the spline
segment of the golden ground-truth knots, so the knots and t0 of pairs_refine_scene.motion() are the truth for every frame and
only the capture time moves.  The baseline to the keyframe grows from 0.10 to 0.42 / 0.32 / 0.22 time units (pairs 0 / 1 / 2).
`frames` adds independent image noise per frame: frame t of pair b = clip(round(frame_bt + noise * n_bt)), n_bt standard normal
draws of a generator seeded by (b, t)."""
import os

import numpy as np

import pairs_refine_scene as sc

# the setting tests/test_pairs_filter_api.py establishes (profiles/r31_pairs_filter.txt): frames, noise in grey levels, the options
T, NOISE = 8, 2.0
OPTS = dict(sigma_i=2.0, prior_rel_sigma=0.05)
START = 0.05                      # the level-0 depths start at truth * (1 +- START)
_FRAMES = {}


def _golden():
    if not _FRAMES:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_scene.npz"))
        _FRAMES.update(frames=np.stack([z["frames%d" % b] for b in range(sc.B)]), caps=np.stack([z["caps%d" % b] for b in range(sc.B)]))
        assert np.array_equal(_FRAMES["frames"][:, 0], sc.scene()["blur"]) and np.array_equal(_FRAMES["caps"][:, 0], sc.motion()["cap"])
    return _FRAMES


def caps(b, T=T):
    """The capture times of pair b's first T frames."""
    return _golden()["caps"][b, :T].copy()


def frames(b, T=T, noise=NOISE):
    """Pair b's first T frames with their image noise, uint8 T x H x W."""
    clean = _golden()["frames"][b, :T].astype(np.float64)
    out = []
    for t in range(T):
        n = np.random.default_rng(1000 + 17 * b + t).standard_normal(clean[t].shape)
        out.append(np.clip(np.rint(clean[t] + noise * n), 0, 255).astype(np.uint8))
    return np.stack(out)


def start_depths(truth, b):
    """The perturbation of test_repeated_steps_lower_cost_and_depth_error: +-5 % by a generator seeded by the pair."""
    return truth * (1.0 + START * np.random.default_rng(3 + b).choice([-1.0, 1.0], truth.size))
