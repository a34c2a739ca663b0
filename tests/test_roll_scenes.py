"""The roll-dominant scenes of roll_scenes.py are usable inputs, checked on the oracle alone (no GPU): at every relative knot
rotation up to pi the warps stay inside the keyframe and the oracle's blocks are finite, and the list of angles takes every branch
of qlog.  These are conditions on the INPUTS of tests/test_gpu_pose_entries.py (the same scenes, by roll_scenes.case_scene), not
tolerances: whatever the kernels are compared against there exists and is not an empty sum."""
import numpy as np
import pytest

import roll_scenes
from roll_scenes import ANGLES, angle_id

# every (k, S) the GPU matrix runs at every angle / at the four angles of its other shapes
ALL_ANGLES_S = {2: (4, 8), 4: (8, 16)}
FEW_ANGLES = [1e-11, 1.1, 3.1, "pi"]
FEW_ANGLES_S = {2: (1, 21, 32), 4: (1, 4, 21, 32)}
F = 3


def _check(orc, sc):
    p, keep = sc.oracle_problem(orc)
    ro = orc.evaluate(p)
    assert np.isfinite(ro["frame_blocks"]).all() and np.isfinite(ro["patch_blocks"]).all()
    assert np.isfinite(ro["H"]).all() and np.isfinite(ro["g"]).all() and ro["cost"] > 0
    valid = orc.count_valid(p)
    assert valid.shape == (sc.F,) and valid.min() >= 0.9 * sc.K * sc.P, valid
    # all three segments of the spline are used (idx = 0, 1, 2)
    assert list(sc.start_idx) == [0, 1, 2] and sc.N == 2 + sc.k


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("angle", ANGLES, ids=angle_id)
def test_roll_scene_is_a_usable_input(orc, angle, k, flip):
    for S in ALL_ANGLES_S[k] + (FEW_ANGLES_S[k] if angle in FEW_ANGLES else ()):
        _check(orc, roll_scenes.case_scene(angle, k, S, F, flip))


@pytest.mark.parametrize("k", [2, 4])
def test_issue_settings_two_frames(orc, k):
    """S = 8, F = 2, with and without alternating knot signs, through roll_scene's own arguments (exact_pi as a flag)."""
    for i, angle in enumerate(ANGLES):
        for flip in (False, True):
            sc = roll_scenes.roll_scene(np.pi if angle == "pi" else angle, k, 8, 2, seed=50 + i, flip=flip, exact_pi=angle == "pi")
            p, keep = sc.oracle_problem(orc)
            ro = orc.evaluate(p)
            assert np.isfinite(ro["frame_blocks"]).all()
            assert orc.count_valid(p).min() >= 0.9 * sc.K * sc.P


def test_knots_are_unit_rolls():
    """The knots are unit quaternions, consecutive ones differ by the asked angle (0.7 .. 1.0 of it) about an axis within the tilt of
    the optical axis, flip only changes signs, and the keypoints are integers inside the disc."""
    for angle in (0.4, 2.9):
        sc = roll_scenes.roll_scene(angle, 4, 8, 3, seed=5)
        fl = roll_scenes.roll_scene(angle, 4, 8, 3, seed=5, flip=True)
        q, qf = sc.knots_R.reshape(-1, 4), fl.knots_R.reshape(-1, 4)
        assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-14)
        assert np.array_equal(qf[0::2], q[0::2]) and np.array_equal(qf[1::2], -q[1::2])
        for a, b in zip(q[:-1], q[1:]):
            rel = roll_scenes.synth.quat_mul(a * [-1, -1, -1, 1], b)
            ang = 2.0 * np.arctan2(np.linalg.norm(rel[:3]), rel[3])
            assert 0.7 * angle - 1e-12 <= ang <= angle + 1e-12
            assert abs(rel[2]) / np.linalg.norm(rel[:3]) > 0.99
        assert np.array_equal(sc.kp_xy, np.rint(sc.kp_xy))
        assert (np.hypot(sc.kp_xy[:, 0] - sc.W / 2, sc.kp_xy[:, 1] - sc.H / 2) <= min(sc.H, sc.W) / 2 - 14 + 1).all()


def _branches_of(angle, k, flip):
    return set(roll_scenes.branches(roll_scenes.case_scene(angle, k, 8, F, flip)))


@pytest.mark.parametrize("k", [2, 4])
def test_angle_list_takes_every_branch_of_qlog(k):
    seen = set()
    for angle in ANGLES:
        for flip in (False, True):
            seen |= _branches_of(angle, k, flip)
    assert seen == {"series", "general+", "general-", "pi"}, seen


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("k", [2, 4])
def test_both_sides_of_the_series_threshold(k, flip):
    """sn = sin^2(a / 2) against 1e-20: every knot pair of the 1e-11 scenes is on the series side, every pair of the 1e-9 scenes on
    the general side; exactly pi is the |w| < 1e-10 branch; an odd knot's negation puts w < 0 on the pairs next to it."""
    assert _branches_of(1e-11, k, flip) == {"series"}
    assert _branches_of(1e-9, k, flip) == ({"general-"} if flip else {"general+"})
    assert _branches_of("pi", k, flip) == {"pi"}
    for angle in (0.05, 1.1, 3.1):
        assert _branches_of(angle, k, flip) == ({"general-"} if flip else {"general+"})
