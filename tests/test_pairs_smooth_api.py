"""mbavo_pairs_smooth_depths without a GPU: the entries exist in the library, the header and the binding, the structs have the sizes
the header states, NULL handles are rejected -- and the specification, restated in numpy (tests/pairs_smooth_ref.py, a brute-force
neighbour search), is held to hand-made cases and to the rendered frames of tests/golden/filter_scene.npz.

The property is established HERE (the figures are in profiles/r33_pairs_smooth.txt): the numpy search of
tests/test_pairs_search_api.py's noise setting (the widest-baseline frame with 2 grey levels of noise, ND = 9 relative candidates on
[0.5, 1.5] from the true depths, a step of 12.5 %) leaves 0 / 2 / 7 of 96 accepted keypoints (pairs 0 / 1 / 2) more than one step
off and a median relative depth error of 0.0139 / 0.0189 / 0.0319.  ONE sweep with SWEEP -- radius 6 = 1.5 cells of the scene's
grid of 4, so that a keypoint has its 8 grid neighbours; max_rel_diff = one candidate step; min_support 3; strength 1; fill 1 -- the
first setting tried, leaves 0 / 0 / 0 and 0.0092 / 0.0105 / 0.0210: ratios of 0.66 / 0.56 / 0.66.  Asserted here: the keypoints over
a step off at least halve (measured: none left) and the median falls to at most MEDIAN_RATIO = 0.83 of what it was (half of the
smallest measured improvement kept as headroom).  tests/test_gpu_pairs_smooth.py asserts the bare inequalities.  Every test here
asks the library for the call first: none passes where mbavo_pairs_smooth_depths does not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_refine_scene as sc
import pairs_smooth_ref as mref

E_ARG = -1
NEW = ["mbavo_pairs_smooth_opts_size", "mbavo_pairs_smooth_size", "mbavo_pairs_smooth_depths", "mbavo_pairs_smooth_stats"]
SWEEP = mref.SWEEP  # the property's setting, shared with tests/test_gpu_pairs_smooth.py
MEDIAN_RATIO = 0.83
NAN = float("nan")


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    """The restatement restates a call of the library: its records are the binding's."""
    assert mbavo.load().mbavo_pairs_smooth_size() == C.sizeof(mbavo.capi.PairsSmooth)


def test_entries_and_struct_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS and name in header
    assert lib.mbavo_pairs_smooth_opts_size() == C.sizeof(capi.PairsSmoothOpts) == 32 + 8 * 4 + 16
    assert lib.mbavo_pairs_smooth_size() == C.sizeof(capi.PairsSmooth) == 24 + 8 + 8
    # the header's own figures, on the lines that open the two structs
    assert "typedef struct mbavo_pairs_smooth_opts {   /* zero-initialise; 80 bytes, no padding */" in header
    assert "struct mbavo_pairs_smooth {                /* one per (pair, level) reported; 40 bytes, no padding */" in header


def test_null_handles_are_rejected(mbavo):
    """(each bad option of a live object: tests/test_gpu_pairs_smooth.py, an object needs a device)"""
    lib, capi = mbavo.load(), mbavo.capi
    out = (capi.PairsSmooth * 1)()
    for o in (mref.opts_struct(capi), mref.opts_struct(capi, radius=0), mref.opts_struct(capi, weights=3), None):
        assert mref.call(lib, None, o, out) == E_ARG
    assert lib.mbavo_pairs_smooth_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert all(callable(getattr(workloads.PairBatch, n)) for n in ("smooth_depths", "smooth_stats"))


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_the_window_is_inclusive_and_a_shared_pixel_is_a_neighbour(mbavo):
    r = 3
    xy = [[10, 10], [10 + r, 10], [10 + r + 1, 10], [10, 10 - r], [10, 10 - r - 1], [10, 10]]
    m = mref.smooth(xy, np.full(6, 2.0), r, min_support=1, max_rel_diff=0.1)
    # 0: (13, 10), (10, 7) and its twin on the same pixel; not (14, 10), not (10, 6).  The window is a square: (13, 10) and (10, 7)
    # are neighbours of each other
    assert m["support"].tolist() == [3, 4, 1, 4, 1, 3]
    assert (m["flags"] == mref.SUPPORTED).all() and m["sum_support"] == 16


def test_a_depth_step_holds_its_edge(mbavo):
    ys, xs = np.meshgrid(np.arange(0, 12), np.arange(0, 16), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    rng = np.random.default_rng(3)
    left = xy[:, 0] < 8
    z = np.where(left, 2.0, 3.0) * (1.0 + rng.uniform(-0.02, 0.02, len(xy)))  # rho 0.5 and 0.33: 33 % apart, max_rel_diff 10 %
    m = mref.smooth(xy, z, 2, min_support=2, max_rel_diff=0.1, strength=1.0, fill=1)
    rho = 1.0 / z
    for side in (left, ~left):
        assert (m["rho"][side] >= rho[side].min()).all() and (m["rho"][side] <= rho[side].max()).all()
    assert (m["flags"] == mref.SUPPORTED).all() and m["num_moved"] > 0.9 * len(xy)


def test_a_planted_outlier_is_filled_or_flagged_and_an_isolated_keypoint_is_an_outlier(mbavo):
    ys, xs = np.meshgrid(np.arange(4, 9), np.arange(4, 9), indexing="ij")
    xy = np.concatenate([np.stack([xs.ravel(), ys.ravel()], 1), [[40, 40]]])
    z = np.full(26, 2.0)
    z[12] = 0.7  # the centre of the 5 x 5 plane
    m = mref.smooth(xy, z, 1, min_support=2, max_rel_diff=0.1, fill=1)
    assert m["flags"][12] == mref.FILLED and m["rho"][12] == 0.5 and m["z_new"][12] == 2.0 and m["support"][12] == 0
    assert m["flags"][25] == mref.OUTLIER and m["z_new"][25] == 2.0 and not m["stands"][25] and _same(m["rho"][25], 0.5)
    # its neighbours do not agree with it: it does not enter their means
    assert (np.delete(m["z_new"], 12) == 2.0).all()
    m = mref.smooth(xy, z, 1, min_support=2, max_rel_diff=0.1, fill=0)
    assert m["flags"][12] == mref.OUTLIER and m["z_new"][12] == 0.7 and _same(m["rho"][12], 1.0 / 0.7) and not m["moved"][12]
    assert (m["num_supported"], m["num_filled"], m["num_outliers"], m["num_valid"]) == (24, 0, 2, 26)
    # an invalid depth: flag 0, NaN, no neighbour of anyone
    z[11] = NAN
    z[13] = -1.0
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.1, fill=1)
    assert m["flags"][[11, 13]].tolist() == [0, 0] and np.isnan(m["rho"][[11, 13]]).all() and m["num_valid"] == 24
    assert m["support"][12] == 0 and m["flags"][12] == mref.FILLED and m["rho"][12] == 0.5


def test_gates_weights_limits_strength_and_support(mbavo):
    xy = [[5, 5], [6, 5], [5, 6], [6, 6]]
    z = np.array([2.0, 2.1, 1.9, 2.05])
    rho = 1.0 / z
    # the intensity gate excludes keypoint 3 from everyone's neighbours, and everyone from its
    I = np.array([100, 104, 96, 140])
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.2, I=I, max_intensity_diff=8)
    assert m["support"].tolist() == [2, 2, 2, 0] and m["flags"][3] == mref.OUTLIER
    assert _same(m["rho"][0], (rho[0] + (rho[1] + rho[2])) / (1.0 + (1.0 + 1.0)))
    # a weight of 0 (and a negative one, and NaN) is skipped as a neighbour; the keypoint itself is still smoothed
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.2, weights=[0.0, 2.0, -1.0, NAN])
    assert m["support"].tolist() == [1, 0, 1, 1] and m["flags"][1] == mref.OUTLIER
    assert _same(m["rho"][0], (0.0 * rho[0] + 1.0 * (2.0 * rho[1])) / (0.0 + 1.0 * 2.0))
    # lambda
    m = mref.smooth(xy[:2], z[:2], 1, min_support=1, max_rel_diff=0.2, strength=0.25)
    assert _same(m["rho"][0], (1.0 * rho[0] + 0.25 * rho[1]) / (1.0 + 0.25 * 1.0))
    # min_support: three neighbours each
    assert (mref.smooth(xy, z, 1, min_support=3, max_rel_diff=0.2)["flags"] == mref.SUPPORTED).all()
    assert (mref.smooth(xy, z, 1, min_support=4, max_rel_diff=0.2, fill=1)["flags"] == mref.OUTLIER).all()
    # a proposal outside [z_min, z_max] does not stand: the class stays, rho' = rho_i, nothing moves
    xy = [[5, 5], [6, 5], [7, 5], [8, 5]]  # (a row: the means differ)
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.2, z_min=2.0)
    n = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.2)
    out = n["z_new"] < 2.0
    assert out.any() and not out.all() and (m["flags"] == mref.SUPPORTED).all()
    assert np.array_equal(m["stands"], ~out) and np.array_equal(m["z_new"][out], z[out]) and all(_same(a, b) for a, b in zip(m["rho"][out], rho[out]))
    assert m["num_moved"] == int((~out).sum())
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.2, z_max=2.0)
    assert np.array_equal(m["stands"], n["z_new"] <= 2.0)


def test_the_sums_run_over_ascending_j(mbavo):
    """1 + 2^-53 + 2^-53 left to right stays 1; 2^-53 + 2^-53 + 1 is 1 + 2^-52."""
    xy = [[5, 5], [6, 5], [5, 6], [6, 6]]
    tiny = 2.0 ** -53
    w = [1.0, 1.0, tiny, tiny]
    z = np.array([1.0, 2.0, 4.0, 4.0])
    m = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.01, weights=w, fill=1)
    back = mref.smooth(xy, z, 1, min_support=1, max_rel_diff=0.01, weights=w, fill=1, order=lambda js: js[::-1])
    # keypoint 0 is filled from 1, 2, 3.  Ascending: SW_N = (1 + tiny) + tiny = 1 and SR_N = (0.5 + tiny / 4) + tiny / 4 = 0.5.
    # Descending: SW_N = (tiny + tiny) + 1 = 1 + 2^-52, SR_N = (tiny / 4 + tiny / 4) + 0.5 = 0.5 (a tie, to even)
    assert m["flags"][0] == mref.FILLED and _same(m["rho"][0], 0.5) and _same(back["rho"][0], 0.5 / (1.0 + 2.0 ** -52))
    assert not _same(back["rho"][0], m["rho"][0])


@pytest.mark.parametrize("b", range(sc.B))
def test_one_sweep_after_the_search_brings_keypoints_back_within_a_step(mbavo, b):
    e, truth, s = mref.noisy_search(mbavo.load(), mbavo.capi, b)
    m = mref.smooth(e["xy"], s["z_new"], **SWEEP)
    (off0, med0), (off1, med1) = mref.figures(s["z_new"], truth, s), mref.figures(m["z_new"], truth, s)
    print("pair %d: over a step off %d -> %d of %d accepted; median relative error %.4f -> %.4f (ratio %.2f); supported %d, filled %d, outliers %d"
          % (b, off0, off1, int(s["accepted"].sum()), med0, med1, med1 / med0, m["num_supported"], m["num_filled"], m["num_outliers"]))
    assert 2 * off1 <= off0
    assert med1 <= MEDIAN_RATIO * med0
