"""mbavo_pairs_search_depths without a GPU: the entries exist in the library, the header and the binding, the structs have the sizes
the header states, NULL handles are rejected -- and the specification, restated in numpy (tests/pairs_search_ref.py on top of
tests/pairs_refine_ref.py), is held to hand-made volumes and to the rendered pairs of tests/pairs_refine_scene.py and
tests/pairs_filter_scene.py (level 0: the host side has no pyramid).

The recovery setting is established HERE (the figures are in profiles/r32_pairs_search.txt): every level-0 keypoint starts at
z = START_Z = 0.4, a fifth of the plane's depth of 2.  T = 8 refinement steps on the widest-baseline frame leave the median
relative error at 0.80 / 0.80 / 0.54 of a start error of 0.80 (pairs 0 / 1 / 2): the refinement cannot repair this start.  T filter
calls (tests/pairs_filter_scene.py's frames and options) end at 0.247 / 0.165 / 0.229.  The search on the widest-baseline frame
(ND = 16 candidates on [0.25, 1.0], min_ratio = 1.05) accepts 96 / 95 / 96 of 96 keypoints and leaves 0.016 / 0.017 / 0.034; T filter
calls after it, seeded from the searched depths, end at 0.0098 / 0.0109 / 0.0183 over the accepted keypoints: 25 / 15 / 12.5 times
below the filter alone.  Asserted here: a factor of FACTOR = 4 (headroom 3 on the smallest measured ratio) and at least MIN_SHARE =
90 % of the keypoints accepted (measured: 99 % at the least).  tests/test_gpu_pairs_search.py asserts the inequality without the
factor.  Every test here asks the library for the call first: none passes where mbavo_pairs_search_depths does not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_filter_ref as fref
import pairs_filter_scene as fs
import pairs_refine_ref as ref
import pairs_refine_scene as sc
import pairs_search_ref as sref

E_ARG = -1
NEW = ["mbavo_pairs_search_opts_size", "mbavo_pairs_search_size", "mbavo_pairs_search_depths", "mbavo_pairs_search_stats"]
# the recovery setting (shared with tests/test_gpu_pairs_search.py, which restates it)
START_Z, ND, RHO_LO, RHO_HI, MIN_RATIO, FACTOR, MIN_SHARE = 0.4, 16, 0.25, 1.0, 1.05, 4.0, 0.9
MAX_OFF_SHARE = 0.15
NAN = float("nan")


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    """The restatement restates a call of the library: its records are the binding's."""
    assert mbavo.load().mbavo_pairs_search_size() == C.sizeof(mbavo.capi.PairsSearch)


def test_entries_and_struct_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS and name in header
    assert lib.mbavo_pairs_search_opts_size() == C.sizeof(capi.PairsSearchOpts) == 16 + 8 * 6 + 16
    assert lib.mbavo_pairs_search_size() == C.sizeof(capi.PairsSearch) == 16 + 8 * 2
    # the header's own figures, on the lines that open the two structs
    assert "typedef struct mbavo_pairs_search_opts {   /* zero-initialise; 80 bytes, no padding */" in header
    assert "struct mbavo_pairs_search {                /* one per (pair, level) reported; 32 bytes, no padding */" in header


def test_null_handles_are_rejected(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    out = (capi.PairsSearch * 1)()
    for o in (sref.opts_struct(capi), sref.opts_struct(capi, num_candidates=1), sref.opts_struct(capi, relative=2), None):
        assert sref.call(lib, None, o, out) == E_ARG
    assert lib.mbavo_pairs_search_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert all(callable(getattr(workloads.PairBatch, n)) for n in ("search_depths", "search_stats"))


def _one(vol, lo=0.5, step=0.25):
    s = sref.select(np.array([vol], np.float64), lo, step)
    return {key: v[0] for key, v in s.items()}


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b))


def test_selection_on_hand_made_volumes(mbavo):
    lo, st = 0.5, 0.25
    # a tie: the lower index wins; c_+ = c_0 puts delta on the clamp's edge, exactly
    s = _one([3.0, 1.0, 1.0, 5.0])
    assert (s["best"], s["num_full"], s["cost_best"], s["cost_second"], s["parabola"]) == (1, 4, 1.0, 5.0, True)
    assert _same(s["rho"], (lo + 1.0 * st) + 0.5 * st) and _same(s["curv"], 2.0 / (st * st))
    s = _one([1.0 + 2.0 ** -52, 1.0, 1.0, 9.0])
    assert s["best"] == 1 and s["parabola"] and abs((s["rho"] - (lo + st)) / st) <= 0.5
    # delta clamped.  With c_0 the lowest cost, |c_- - c_+| <= den in exact arithmetic, so delta leaves [-0.5, 0.5] by rounding
    # only, and only upwards: with c_+ = c_0 = 1 and c_- = 2^54 + 4 the numerator c_- - 1 rounds up to 2^54 + 4 while den =
    # (c_- - 2) + 1 rounds twice, down to 2^54, and the unclamped quotient is 0.5 (1 + 2^-52).  (Downwards c_- > c_0 strictly -- a
    # tie goes to the lower index -- so den exceeds c_+ - c_- before one monotone rounding of each, and -0.5 is never passed.)
    # The clamp is what changes the value here (the selection is a pure function: lo = -step puts rho_best at 0, where one
    # rounding of delta is not lost in rho*)
    vol = [2.0 ** 54 + 4.0, 1.0, 1.0, 9.0]
    unclamped = 0.5 * (vol[0] - vol[2]) / ((vol[0] - 2.0 * vol[1]) + vol[2])
    assert unclamped > 0.5
    s = _one(vol, lo=-st, step=st)
    assert s["best"] == 1 and s["parabola"] and _same(s["rho"], (-st + st) + 0.5 * st) and not _same(s["rho"], (-st + st) + unclamped * st)
    # best at either end: no parabola, curv 0, rho on the candidate
    s = _one([1.0, 2.0, 3.0])
    assert (s["best"], s["cost_second"], s["parabola"], s["curv"]) == (0, 3.0, False, 0.0) and _same(s["rho"], lo)
    s = _one([3.0, 2.0, 1.0])
    assert (s["best"], s["cost_second"], s["parabola"], s["curv"]) == (2, 3.0, False, 0.0) and _same(s["rho"], lo + 2.0 * st)
    # a neighbour that is not full
    s = _one([NAN, 1.0, 2.0, 3.0])
    assert (s["best"], s["num_full"], s["cost_second"], s["parabola"], s["curv"]) == (1, 3, 3.0, False, 0.0) and _same(s["rho"], lo + st)
    s = _one([4.0, 1.0, NAN, 3.0])
    assert (s["best"], s["cost_second"], s["parabola"]) == (1, 3.0, False)
    # den <= 0 (2 c_0 overflows)
    s = _one([1.5e308, 1e308, 1.6e308])
    assert (s["best"], s["parabola"], s["curv"]) == (1, False, 0.0) and _same(s["rho"], lo + st) and np.isnan(s["cost_second"])
    # all candidates not full
    s = _one([NAN, NAN, NAN])
    assert (s["best"], s["num_full"], s["curv"]) == (-1, 0, 0.0) and np.isnan(s["rho"]) and np.isnan(s["cost_best"]) and np.isnan(s["cost_second"])
    # a runner-up that exists only adjacent to the best
    s = _one([2.0, 1.0, 3.0])
    assert s["best"] == 1 and s["parabola"] and np.isnan(s["cost_second"])
    # the runner-up is the lowest NON-adjacent cost, behind two cheaper neighbours and a third cheaper candidate that is the best
    s = _one([9.0, 2.0, 1.0, 3.0, 8.0, 7.0])
    assert (s["best"], s["cost_second"]) == (2, 7.0)
    # ND = 2
    s = _one([2.0, 1.0])
    assert (s["best"], s["parabola"], s["curv"]) == (1, False, 0.0) and np.isnan(s["cost_second"]) and _same(s["rho"], lo + st)
    # acceptance: the ratio test turns a NaN runner-up away, min_curv > 0 turns a keypoint without a parabola away
    sel = sref.select(np.array([[2.0, 1.0, 3.0, NAN], [1.0, 2.0, 3.0, NAN], [5.0, 1.0, 5.0, 1.04]]), lo, st)
    assert sref.accept(sel)[0].tolist() == [True, True, True]
    assert sref.accept(sel, min_ratio=1.05)[0].tolist() == [False, True, False]
    assert sref.accept(sel, min_curv=1.0)[0].tolist() == [True, False, True]
    assert sref.accept(sel, z_min=1.1)[0].tolist() == [True, True, True] and sref.accept(sel, z_max=1.5)[0].tolist() == [True, False, True]


def _entry(b, z=None, frame=None, noise=fs.NOISE):
    e = sc.entry(b)
    if frame is not None:
        e["curs"] = [np.ascontiguousarray(fs.frames(b, noise=noise)[frame])]
        e["cap"] = np.array([fs.caps(b)[frame]])
    if z is not None:
        e["z"] = np.asarray(z, np.float64)
    return e


@pytest.mark.parametrize("b", range(sc.B))
def test_a_candidate_costs_what_the_refinement_says_at_its_depth(mbavo, b):
    lib, capi = mbavo.load(), mbavo.capi
    e = _entry(b)
    for relative, lo, hi in ((0, 0.3, 0.8), (1, 0.7, 1.4)):
        s = sref.search(lib, capi, e, e["k"], e["K"], 5, lo, hi, relative)
        pl = ref.poses(lib, capi, e, e["k"])
        assert s["num_searched"] > 0
        for d in range(5):
            D = 1.0 / ((lo / e["z"] if relative else lo) + float(d) * s["step"])
            assert np.array_equal(D.view(np.uint64), s["D"][:, d].view(np.uint64))
            r = ref.keypoints(e, pl, z=D)
            assert np.array_equal(np.isnan(s["volume"][:, d]), ~r["full"])
            assert np.array_equal(s["volume"][r["full"], d].view(np.uint64), r["cost"][r["full"]].view(np.uint64))


@pytest.mark.parametrize("b", range(sc.B))
def test_with_the_truth_among_the_candidates_the_search_stays_within_a_step(mbavo, b):
    """relative = 1 from the true depths with an odd ND puts rho_true on the middle candidate.  The widest-baseline frame as it was
    rendered, without the image noise of the filter tests: noise moves the minimum of the cost itself (by more than a step of
    12.5 % on 2 and 7 keypoints of pairs 1 and 2 at 2 grey levels), which is the measurement's doing, not the selection's."""
    lib, capi = mbavo.load(), mbavo.capi
    e = _entry(b, frame=fs.T - 1, noise=0.0)
    truth = e["z"].copy()
    s = sref.search(lib, capi, e, e["k"], e["K"], 9, 0.5, 1.5, 1)
    acc = s["accepted"]
    off = np.abs(s["rho"][acc] - 1.0 / truth[acc]) / s["step"][acc]
    print("pair %d: %d of %d accepted, |rho* - rho_true| / step: median %.3f, max %.3f" % (b, acc.sum(), acc.size, np.median(off), off.max()))
    assert acc.sum() >= MIN_SHARE * acc.size and (off <= 1.0).all()


@pytest.mark.parametrize("b", range(sc.B))
def test_under_image_noise_few_accepted_keypoints_leave_the_true_step(mbavo, b):
    """The same search on the widest-baseline frame WITH the filter tests' noise of 2 grey levels, where the minimum of the cost
    itself moves.  Measured on the restatement (profiles/r32_pairs_search.txt): all 96 keypoints accepted, 0 / 2 / 7 of them
    (pairs 0 / 1 / 2) more than one step of 12.5 % off, at most 0.74 / 2.1 / 4.0 steps, median 0.11 / 0.15 / 0.26 of a step.  Asserted: at
    most MAX_OFF_SHARE = 15 % of the accepted keypoints more than one step off (twice the worst measured share of 7.3 %) and a
    median within half a step (twice the worst measured; what the nearest candidate alone would give): a selection that went
    wrong under noise would show in either."""
    lib, capi = mbavo.load(), mbavo.capi
    e = _entry(b, frame=fs.T - 1)
    truth = e["z"].copy()
    s = sref.search(lib, capi, e, e["k"], e["K"], 9, 0.5, 1.5, 1)
    acc = s["accepted"]
    off = np.abs(s["rho"][acc] - 1.0 / truth[acc]) / s["step"][acc]
    print("pair %d with noise: %d of %d accepted, %d more than a step off, |rho* - rho_true| / step: median %.3f, max %.3f"
          % (b, acc.sum(), acc.size, (off > 1.0).sum(), np.median(off), off.max()))
    assert acc.sum() >= MIN_SHARE * acc.size
    assert (off > 1.0).sum() <= MAX_OFF_SHARE * acc.sum() and np.median(off) <= 0.5


def _filtered(mbavo, b, z):
    """T filter calls with apply = 1 from depths z, seeded in the first (tests/test_pairs_filter_api.py's sequence)."""
    lib, capi = mbavo.load(), mbavo.capi
    state = None
    for t in range(fs.T):
        e = _entry(b, z, frame=t)
        r = ref.keypoints(e, ref.poses(lib, capi, e, e["k"]))
        before = fref.seed(z, fs.OPTS["prior_rel_sigma"]) if t == 0 else state
        f = fref.fuse(z, r["g"], r["h"], r["full"], before, **fs.OPTS)
        state, z = f["state"], f["z_new"]
    return z


@pytest.mark.parametrize("b", range(sc.B))
def test_the_search_recovers_what_refinement_and_filter_cannot(mbavo, b):
    lib, capi = mbavo.load(), mbavo.capi
    truth = sc.entry(b)["z"]
    z0 = np.full(truth.size, START_Z)
    err = lambda z, sel=slice(None): float(np.median(np.abs(z[sel] / truth[sel] - 1.0)))
    z_ref = z0
    for _ in range(fs.T):  # the refinement alone, on the widest-baseline frame
        e = _entry(b, z_ref, frame=fs.T - 1)
        r = ref.keypoints(e, ref.poses(lib, capi, e, e["k"]))
        z_ref = ref.step(e["z"], r["g"], r["h"], r["full"])[1]
    z_fil = _filtered(mbavo, b, z0)
    e = _entry(b, z0, frame=fs.T - 1)
    s = sref.search(lib, capi, e, e["k"], e["K"], ND, RHO_LO, RHO_HI, 0, min_ratio=MIN_RATIO)
    acc = s["accepted"]
    z_both = _filtered(mbavo, b, s["z_new"])
    print("pair %d: start %.4f; %d refinement steps %.4f; %d filter calls %.4f; search accepts %d of %d and leaves %.4f; search + filter %.4f "
          "(filter alone on the accepted %.4f, ratio %.1f)" % (b, err(z0), fs.T, err(z_ref), fs.T, err(z_fil), acc.sum(), acc.size, err(s["z_new"], acc),
                                                              err(z_both, acc), err(z_fil, acc), err(z_fil, acc) / err(z_both, acc)))
    assert err(z_ref) > 0.5 * err(z0)                       # the start is one the refinement cannot repair
    assert acc.sum() >= MIN_SHARE * acc.size                # the median hides no rejections
    assert FACTOR * err(z_both, acc) < err(z_fil, acc)
