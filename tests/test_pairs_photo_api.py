"""mbavo_pairs_match_brightness without a GPU: the entries exist in the library, the header and the binding, the structs have the
sizes the header states, NULL handles are rejected -- and the specification, restated in numpy (tests/pairs_photo_ref.py), has the
two properties the call is for, on the rendered frames of tests/golden/filter_scene.npz (tests/pairs_filter_scene.py: three pairs,
frames FRAMES of each, without image noise) at their TRUE poses and depths, the blurred frame B replaced by clip(rint(a* B + b*)):

  1. the fit recovers (a*, b*) for SETTINGS;
  2. after the correction with the fitted (a, b), cost_after < cost_before on every pair with (a*, b*) != (1, 0).

The tolerance of 1 (TOL_GAIN, relative; TOL_OFFSET, grey levels) is measured here, from the restatement alone: the worst error over
the settings, pairs and frames, doubled as margin for other poses (profiles/r42_pairs_photo.txt lists the figures).  The error is
not rounding: the frames are rounded to whole grey levels and clipped at 255 (1.3 B - 20 saturates where B > 211), and the blurred
frame was rendered with 8 samples while the evaluation synthesises it with 3.
The last test holds step 5's normal equations, in the header's uncentred float64 form, to a centred long-double solution at the
lowest variance and highest mean the stage admits.
Every test here asks the library for the call first: none passes where mbavo_pairs_match_brightness does not exist."""
import ctypes as C

import numpy as np
import pytest

import pairs_filter_scene as fs
import pairs_photo_ref as pref
import pairs_refine_ref as ref
import pairs_refine_scene as sc

E_ARG = -1
NEW = ["mbavo_pairs_photo_opts_size", "mbavo_pairs_photo_size", "mbavo_pairs_match_brightness", "mbavo_pairs_photo_stats"]
SETTINGS = [(1.3, -20.0), (0.7, 15.0), (1.0, 0.0)]
FRAMES = (0, 3, 7)
WORST_GAIN, WORST_OFFSET = 0.04445, 6.691   # (1.3, -20), pair 2, frame 0 -- (0.7, +15): 0.0043, 0.42; (1, 0): 0.0050, 0.66.  The worst |a - a*| / a* and |b - b*| measured over SETTINGS x pairs x FRAMES
TOL_GAIN, TOL_OFFSET = 2 * WORST_GAIN, 2 * WORST_OFFSET
CAP = 96                              # the keypoint capacity the sums are tiled for: the entries' own K
_ITEMS = {}


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    """The restatement restates a call of the library: its records are the binding's."""
    assert mbavo.load().mbavo_pairs_photo_size() == C.sizeof(mbavo.capi.PairsPhoto)


def test_entries_struct_sizes_and_defaults(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(mbavo.HEADER_PATH).read() if hasattr(mbavo, "HEADER_PATH") else None
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert header is None or name in header
    assert lib.mbavo_pairs_photo_opts_size() == C.sizeof(capi.PairsPhotoOpts) == 4 * 4 + 8 * 4 + 16
    assert lib.mbavo_pairs_photo_size() == C.sizeof(capi.PairsPhoto) == 16 + 8 * 4
    # no padding: the fields fill the structs
    assert sum(C.sizeof(t) for _, t in capi.PairsPhotoOpts._fields_) == 64 and sum(C.sizeof(t) for _, t in capi.PairsPhoto._fields_) == 48
    assert [n for n, _ in capi.PairsPhotoOpts._fields_][-1] == "reserved" and bytes(capi.PairsPhotoOpts()) == bytes(64)
    # the defaults the header states for 0, as the restatement fills them in
    assert pref.DEFAULTS == dict(rounds=3, min_pixels=64, min_var=4.0, gain_min=0.25, gain_max=4.0) and pref.DEGENERATE == 1


def test_null_handles_are_rejected(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    o, out = capi.PairsPhotoOpts(), (capi.PairsPhoto * 1)()
    assert lib.mbavo_pairs_match_brightness(None, C.byref(o), out) == E_ARG
    assert lib.mbavo_pairs_photo_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_method_exists(mbavo):
    from mba_vo_amd import workloads
    assert callable(workloads.PairBatch.match_brightness) and callable(workloads.PairBatch.photo_stats)


def _entry(b, t, a, bb):
    """Pair b's level-0 entry at frame t of the filter scene, its blurred frame as a camera with gain a and offset bb took it."""
    e = sc.entry(b)
    e["cap"] = fs.caps(b)[t:t + 1].copy()
    e["curs"] = [pref.exposed(fs.frames(b, noise=0.0)[t], a, bb)]
    return e


def _fitted(mbavo, b, t, setting):
    """(entry, items, fit) of one case, made once."""
    key = (b, t, setting)
    if key not in _ITEMS:
        lib, capi = mbavo.load(), mbavo.capi
        e = _entry(b, t, *SETTINGS[setting])
        assert e["K"] == CAP
        s, c, ok = pref.items(e, ref.poses(lib, capi, e, e["k"]))
        _ITEMS[key] = (e, (s, c, ok), pref.fit_items(s, c, ok, e["P"], CAP, e["huber"]))
    return _ITEMS[key]


def test_the_fit_recovers_gain_and_offset(mbavo):
    worst = [0.0, 0.0]
    for setting, (a, bb) in enumerate(SETTINGS):
        for b in range(sc.B):
            for t in FRAMES:
                e, _, r = _fitted(mbavo, b, t, setting)
                assert r["status"] == 0 and r["num_full"] > e["K"] // 2 and r["num_pixels"] == r["num_full"] * e["P"]
                eg, eo = abs(r["gain"] - a) / a, abs(r["offset"] - bb)
                worst = [max(worst[0], eg), max(worst[1], eo)]
                print("(%.1f, %+.0f) pair %d frame %d: gain %.5f offset %+.4f  errors %.3g %.3g  cost %.6g -> %.6g  full %d"
                      % (a, bb, b, t, r["gain"], r["offset"], eg, eo, r["cost_before"], r["cost_after"], r["num_full"]))
    print("worst gain error %.4g (tolerance %.4g), worst offset error %.4g (tolerance %.4g)" % (worst[0], TOL_GAIN, worst[1], TOL_OFFSET))
    assert worst[0] <= TOL_GAIN and worst[1] <= TOL_OFFSET


def test_the_correction_lowers_the_cost(mbavo):
    """The restated correction applied to the exposed frame with the FITTED (a, b); the cost of the fit residuals under (1, 0) on
    the corrected frame (a second call's cost_before) lies below the first call's cost_before."""
    lib, capi = mbavo.load(), mbavo.capi
    for setting, (a, bb) in enumerate(SETTINGS[:2]):
        for b in range(sc.B):
            for t in FRAMES:
                e, _, r = _fitted(mbavo, b, t, setting)
                assert r["cost_after"] < r["cost_before"]
                e2 = dict(e, curs=[pref.correct(e["curs"][0], r["gain"], r["offset"])])
                r2 = pref.fit(lib, capi, e2, e["k"], CAP)
                print("(%.1f, %+.0f) pair %d frame %d: cost %.6g, under the fit %.6g, on the corrected frame %.6g (what is left: %.5f %+.4f)"
                      % (a, bb, b, t, r["cost_before"], r["cost_after"], r2["cost_before"], r2["gain"], r2["offset"]))
                assert r2["cost_before"] < r["cost_before"]


def test_degenerate_and_off_knots_records(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    e, (s, c, ok), _ = _fitted(mbavo, 0, 0, 2)
    P = e["P"]
    # a constant keyframe: no variance of s
    r = pref.fit_items(np.full_like(s, 100.0), c, ok, P, CAP, e["huber"])
    assert (r["status"], r["gain"], r["offset"]) == (pref.DEGENERATE, 1.0, 0.0) and r["cost_after"] == r["cost_before"]
    # no keypoints, too few pixels, a gain outside the window
    r = pref.fit_items(s[:0], c[:0], ok[:0], P, CAP, e["huber"])
    assert (r["status"], r["num_full"], r["num_pixels"], r["cost_before"], r["cost_after"]) == (pref.DEGENERATE, 0, 0, 0.0, 0.0)
    assert pref.fit_items(s[:4], c[:4], ok[:4], P, CAP, e["huber"])["status"] == (pref.DEGENERATE if ok[:4].all(1).sum() * P < 64 else 0)
    assert pref.fit_items(s, 1.3 * c, ok, P, CAP, e["huber"], gain_max=1.2)["status"] == pref.DEGENERATE
    assert pref.fit_items(s, 1.3 * c, ok, P, CAP, e["huber"])["status"] == 0
    # off the knots
    far = dict(e, t0=100.0)
    r = pref.fit(lib, capi, far, e["k"], CAP)
    assert (r["status"], r["num_keypoints"], r["num_full"], r["num_pixels"]) == (pref.E_RANGE, e["K"], 0, 0)
    assert all(np.isnan(r[key]) for key in ("gain", "offset", "cost_before", "cost_after"))


def test_the_correction_is_the_formula():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(pref.correct(img, 1.0, 0.0), img)
    got = pref.correct(img, 2.0, 1.0)      # (v - 1) / 2: halves round to even, -0.5 to 0
    assert got[0, 0] == 0 and got[0, 2] == 0 and got[0, 4] == 2 and got[0, 6] == 2 and got[0, 8] == 4
    assert pref.correct(img, 0.5, 0.0).max() == 255 and pref.correct(img, 1.0, 300.0).max() == 0
    pyr = pref.corrected_pyramid(np.tile(img, (3, 4)), 1.3, -20.0, 3)
    assert [p.shape for p in pyr] == [(48, 64), (24, 32), (12, 16)] and np.array_equal(pyr[0], pref.correct(np.tile(img, (3, 4)), 1.3, -20.0))


NORMAL_WORST = (1.08e-11, 2.24e-10)  # the largest errors of gain and offset measured here on the CPU (the test's docstring)
NORMAL_LIMIT = 1e-9        # the stage's own bound (tests/test_gpu_pairs_photo_options.py): its definition must be tighter


def _low_variance_items(seed):
    """K x P restated items with the worst cancellation the stage admits: keyframe intensities of mean 250 and a weighted variance
    just above min_var = 4 grey levels squared (whole grey levels, as blends of equal taps give them, and thirds, as S = 3 gives),
    12 500 keypoints of 8 pixels, a current frame of gain 0.9 and offset 12 with noise and a tenth of gross outliers for Huber."""
    rng = np.random.default_rng(seed)
    K, P = 12500, 8
    s = 250.0 + np.rint(3.0 * rng.normal(0.0, 2.06, (K, P))) / 3.0
    c = np.rint(0.9 * s + 12.0 + rng.normal(0.0, 3.0, (K, P)))
    c = np.where(rng.uniform(size=(K, P)) < 0.1, c + rng.choice([-60.0, 45.0], (K, P)), c)
    return np.minimum(s, 255.0), np.clip(c, 0.0, 255.0), K, P


def test_the_normal_equations_against_centred_long_double():
    """Step 5 as the header writes it -- det = n Sxx - Sx Sx, a = (n Sxy - Sx Sy) / det, b = (Sy - a Sx) / n, in float64 on the six
    float64 sums in the kernel's order (pairs_photo_ref.sums, solve) -- against the centred weighted least-squares solution in
    np.longdouble on the same items and weights: a = sum ww (s - ms)(c - mc) / sum ww (s - ms)^2, b = mc - a ms.  With a mean of 250
    and a variance of 4 the uncentred form loses log2(250^2 / 4) = 14 bits to cancellation, the worst the stage admits (a lower
    variance is degenerate).  Measured here on the CPU over three seeds and the rounds 0 .. 2 of the reweighting: the largest
    relative error of the gain 1.08e-11, of the offset (relative to max(|offset|, 1 grey level)) 2.24e-10 (NORMAL_WORST: the offset
    takes the gain's error times the mean, 250).  Allowed: 8 x those figures; and the errors themselves must stay under 1e-9, the bound
    the device is held to against this form, so that the stage's bound is not tighter than its definition and the header needs no note."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    worst = [0.0, 0.0]
    L = np.longdouble
    for seed in (1, 2, 3):
        s, c, K, P = _low_variance_items(seed)
        full = np.ones(K, bool)
        a, b = 1.0, 0.0
        for r in range(3):
            v = pref.sums(s, c, full, a, b, 10.0, P, K)
            det, a1, b1 = pref.solve(*v[:5])
            w = ref.huber(c - (a * s + b), 10.0)[0]
            ww = (w * w).astype(L)
            sl, cl = s.astype(L), c.astype(L)
            n = ww.sum()
            ms, mc = (ww * sl).sum() / n, (ww * cl).sum() / n
            var = (ww * (sl - ms) * (sl - ms)).sum() / n
            al = (ww * (sl - ms) * (cl - mc)).sum() / (ww * (sl - ms) * (sl - ms)).sum()
            bl = mc - al * ms
            ea, eb = float(abs(L(a1) - al) / abs(al)), float(abs(L(b1) - bl) / max(abs(bl), L(1.0)))
            print("seed %d round %d: n %.1f mean %.3f weighted variance %.4f (det / n^2 %.4f)  gain %.15f offset %+.12f  errors %.3g %.3g"
                  % (seed, r, float(n), float(ms), float(var), det / (v[0] * v[0]), a1, b1, ea, eb))
            assert 4.0 < float(var) < 4.6 and 249.0 < float(ms) < 251.0 and K * P == 100000 and det > (4.0 * v[0]) * v[0]
            assert 0.05 < float((w != 1.0).mean()) < 0.95
            worst = [max(worst[0], ea), max(worst[1], eb)]
            a, b = a1, b1
    print("normal equations against centred long double: worst gain error %.3g (allowed %.3g), worst offset error %.3g (allowed %.3g)"
          % (worst[0], 8 * NORMAL_WORST[0], worst[1], 8 * NORMAL_WORST[1]))
    assert worst[0] <= 8 * NORMAL_WORST[0] and worst[1] <= 8 * NORMAL_WORST[1]
    assert max(worst) < NORMAL_LIMIT
