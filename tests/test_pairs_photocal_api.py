"""mbavo_pairs_set_photometric and its companions without a GPU: the entries exist in the library, the header and the binding, the
options have the size the header states, NULL handles are rejected, mbavo_photometric_table equals the numpy restatement
(tests/pairs_photocal_ref.py) bit for bit and rejects what the header names -- and the restatement has the properties the feature
exists for, on the rendered frames of tests/golden/filter_scene.npz (three pairs, 64 x 48, frames FRAMES of each, without image
noise) at their TRUE poses and depths, keyframe and blurred frame passed through a synthetic sensor raw = clip(rint(U(I V))): V a
radial fall-off to CORNER at the corners, U the gamma-1/2.2 response, the calibration the matching G and V with scale = min V.

  1. the corrected frames lie closer to scale * I than the raw frames do, on every frame of every pair, within TOL grey levels;
  2. the level-0 Huber cost summed over each pair's keypoints is lower after the calibration than before, on every pair and frame.

TOL is measured here, from the restatement alone: the worst |corrected - scale I| over keyframes and frames is WORST = 1.0 grey
level, doubled as the brightness tests double theirs (profiles/r43_pairs_photocal.txt lists the figures).  It is quantisation, not
rounding of the arithmetic: the sensor stores whole grey levels of a gamma-encoded value -- one raw level near white spans 2.2
levels of irradiance, divided by V -- and the object stores whole grey levels again.
The first sensor tried (CORNER = 0.5, gamma 2.2) has both properties; no other setting was needed.
Every test here asks the library for the new entries first: none passes where mbavo_pairs_set_photometric does not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_filter_scene as fs
import pairs_photocal_ref as pc
import pairs_refine_ref as ref
import pairs_refine_scene as sc
import pairs_undistort_ref as uref

E_ARG = -1
NEW = ["mbavo_photometric_table", "mbavo_pairs_photocal_opts_size", "mbavo_pairs_set_photometric", "mbavo_pairs_clear_photometric",
       "mbavo_pairs_photocal_stats", "mbavo_photometric_u8_batch"]
FRAMES = (0, 3, 7)
CORNER, GAMMA = 0.5, 2.2
WORST = 1.0          # grey levels: the largest |corrected - scale I| measured here over 3 keyframes and 9 frames
TOL = 2 * WORST


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    """The restatement restates calls of the library: its options are the binding's."""
    assert mbavo.load().mbavo_pairs_photocal_opts_size() == C.sizeof(mbavo.capi.PairsPhotocalOpts)


def _table(lib, G, scale, fill=np.nan):
    out = np.full(256, fill, np.float32)
    g = None if G is None else np.ascontiguousarray(G, np.float64)
    rc = lib.mbavo_photometric_table(None if g is None else g.ctypes.data_as(C.POINTER(C.c_double)), float(scale), out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out


def _curves():
    flat = np.concatenate([np.zeros(20), np.linspace(0.0, 3.5, 200), np.full(36, 3.5)])  # flat ends: saturated codes share a value
    return dict(identity=None, gamma=pc.gamma_G(GAMMA), flat_ends=flat, offset_log=np.log1p(np.arange(256.0)) - 7.0)


def test_entries_struct_size_and_null_handles(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert "int %s(" % name in header
    assert "} mbavo_pairs_photocal_opts;" in header
    assert lib.mbavo_pairs_photocal_opts_size() == C.sizeof(capi.PairsPhotocalOpts) == 8 + 4 + 4 * 5
    assert sum(C.sizeof(t) for _, t in capi.PairsPhotocalOpts._fields_) == 32 and bytes(capi.PairsPhotocalOpts()) == bytes(32)
    assert [n for n, _ in capi.PairsPhotocalOpts._fields_] == ["scale", "v_min", "reserved"]
    assert lib.mbavo_abi_version() == 3  # the change only adds
    o = capi.PairsPhotocalOpts()
    assert lib.mbavo_pairs_set_photometric(None, 1, None, None, C.byref(o)) == E_ARG
    assert lib.mbavo_pairs_clear_photometric(None) == E_ARG
    assert lib.mbavo_pairs_photocal_stats(None, (C.c_longlong * 3)()) == E_ARG
    lut = np.zeros(256, np.float32)
    assert lib.mbavo_photometric_u8_batch(None, 1, None, 4, 4, 1, lut.ctypes.data_as(C.POINTER(C.c_float)), None, None, None) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert mbavo.load().mbavo_pairs_photocal_opts_size() == 32
    for name in ("set_photometric", "clear_photometric", "photocal_stats"):
        assert callable(getattr(workloads.PairBatch, name))
    assert callable(workloads.photometric_u8_batch) and callable(workloads.photometric_table)
    rc, lut = workloads.photometric_table(None, 1.0)
    assert rc == 0 and np.array_equal(lut, np.arange(256, dtype=np.float32))


def test_the_table_equals_the_restatement_bit_for_bit(mbavo):
    lib = mbavo.load()
    for name, G in _curves().items():
        for scale in (1.0, 0.5, 0.37):
            rc, got = _table(lib, G, scale)
            want = pc.table(G, scale)
            assert rc == 0 and want is not None and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, scale)
            assert got[0] == 0.0 and got[255] == np.float32(np.float64(scale) * 255.0) and (np.diff(got) >= 0).all()
    rc, got = _table(lib, None, 1.0)
    assert rc == 0 and np.array_equal(got, np.arange(256, dtype=np.float32))  # lut[i] == i exactly
    rc, got = _table(lib, np.arange(256.0) * 3.0 + 11.0, 1.0)  # any affine copy of the identity is the identity, to the last bit or so
    assert rc == 0 and np.abs(got - np.arange(256)).max() <= 255 * 2.0 ** -23


def test_every_rejection_leaves_the_output_untouched(mbavo):
    lib = mbavo.load()
    ok = pc.gamma_G(GAMMA)
    bad = {}
    for tag, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        bad[tag] = ok.copy()
        bad[tag][77] = v
    bad["constant"] = np.full(256, 3.0)
    bad["last below first"] = ok[::-1].copy()
    bad["one decreasing step"] = ok.copy()
    bad["one decreasing step"][100] = ok[99] - 1e-9
    for tag, G in bad.items():
        rc, out = _table(lib, G, 1.0, fill=-7.0)
        assert rc == E_ARG and (out == -7.0).all() and pc.table(G, 1.0) is None, tag
    for scale in (0.0, -0.5, 1.0 + 2.0 ** -52, 2.0, np.nan, np.inf):
        for G in (ok, None):
            rc, out = _table(lib, G, scale, fill=-7.0)
            assert rc == E_ARG and (out == -7.0).all() and pc.table(G, scale) is None, scale
    assert lib.mbavo_photometric_table(ok.ctypes.data_as(C.POINTER(C.c_double)), 1.0, None) == E_ARG
    # equal neighbours and the smallest admissible scale pass
    assert _table(lib, np.repeat(np.arange(128.0), 2), 1.0)[0] == 0 and _table(lib, ok, 5e-324)[0] == 0


def test_identity_calibration_is_todays_path(mbavo):
    assert mbavo.load().mbavo_pairs_photocal_opts_size() == 32
    rng = np.random.default_rng(5)
    ident = pc.table(None, 1.0)
    img = rng.integers(0, 256, (11, 19), dtype=np.uint8)
    assert np.array_equal(pc.pinhole(img, ident), img)
    assert np.array_equal(pc.pinhole(img, ident, np.ones(img.shape, np.float32)), img)
    intr = uref.intrinsics(9, 17)
    for dist in (uref.DIST_OUTSIDE, uref.DIST_INSIDE, uref.DIST_NONE):
        m = uref.undistort_map(uref.intrinsics(11, 19), dist, intr, 9, 17)
        m[0, 0] = (np.nan, 1.0)
        m[1, 1] = (-0.5, -0.5)
        m[2, 2] = (18.5, 10.5)
        assert np.array_equal(pc.remap(img, m, ident), uref.remap_u8(img, m))
        assert np.array_equal(pc.remap(img, m, ident, np.ones(img.shape, np.float32)), uref.remap_u8(img, m))


def test_the_tap_is_exact_and_the_inverse_is_the_formula(mbavo):
    assert mbavo.load().mbavo_pairs_photocal_opts_size() == 32
    rng = np.random.default_rng(6)
    lut = pc.table(pc.gamma_G(GAMMA), 0.61)
    V = rng.uniform(0.03, 1.0, 4096).astype(np.float32)
    inv = pc.inverse_vignette(V)
    raw = rng.integers(0, 256, 4096).astype(np.uint8)
    t = pc.tap(lut, inv, raw)
    # float64 of the float product against the double product: the 48-bit product of two 24-bit significands fits 53 bits
    exact = np.array([float(np.longdouble(a) * np.longdouble(b)) for a, b in zip(lut[raw], inv)])
    assert np.finfo(np.longdouble).eps < 2.0 ** -60 and np.array_equal(t, exact)
    assert ((V < pc.V_MIN) == (inv == 0)).all() and (V < pc.V_MIN).any() and (t.max() > 255.0)
    special = pc.inverse_vignette(np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 0.0625, 0.06249, 1.0, 3.0], np.float32))
    assert np.array_equal(special, np.array([0, 0, 0, 0, 0, 16.0, 0, 1.0, np.float32(1.0) / np.float32(3.0)], np.float32))
    assert pc.inverse_vignette(np.array([0.01], np.float32), 0.005)[0] == np.float32(1.0) / np.float32(0.01)
    assert np.array_equal(pc.to_u8(np.array([0.0, 0.49, 0.5, 254.5, 255.0, 300.0, 1e30, np.nan])), np.array([0, 0, 1, 255, 255, 255, 255, 255], np.uint8))


def _sensor_case():
    V = pc.radial_vignette(sc.H, sc.W, CORNER)
    scale = float(V.min())
    return V, scale, pc.table(pc.gamma_G(GAMMA), scale), pc.inverse_vignette(V)


def _cost(lib, capi, b, t, key, cur):
    """The level-0 Huber cost of pair b's keypoints at frame t of the filter scene, keyframe and current frame as given."""
    e = sc.entry(b)
    e["cap"] = fs.caps(b)[t:t + 1].copy()
    e["ref"], e["grad"], e["curs"] = np.ascontiguousarray(key), sc.gradient(key), [np.ascontiguousarray(cur)]
    r = ref.keypoints(e, ref.poses(lib, capi, e, e["k"]))
    return float(r["cost"].sum()), int(r["full"].sum())


def test_calibration_restores_irradiance_and_lowers_the_cost(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    V, scale, lut, inv = _sensor_case()
    assert abs(scale - CORNER) < 1e-6 and abs(float(V.max()) - 1.0) < 2e-3
    worst = 0.0
    for b in range(sc.B):
        key = sc.scene()["sharp"][b]
        raw_key = pc.sensor(key, V, GAMMA)
        cal_key = pc.pinhole(raw_key, lut, inv)
        images = [("keyframe", key, raw_key, cal_key)]
        for t in FRAMES:
            fr = fs.frames(b, noise=0.0)[t]
            raw_fr = pc.sensor(fr, V, GAMMA)
            images.append(("frame %d" % t, fr, raw_fr, pc.pinhole(raw_fr, lut, inv)))
        for name, I, raw, cal in images:
            want = scale * I.astype(np.float64)
            e_cal, e_raw = np.abs(cal - want), np.abs(raw - want)
            print("pair %d %-8s: |corrected - scale I| mean %.4f worst %.2f   |raw - scale I| mean %.2f worst %.1f"
                  % (b, name, e_cal.mean(), e_cal.max(), e_raw.mean(), e_raw.max()))
            assert e_cal.mean() < e_raw.mean() and e_cal.max() <= TOL
            worst = max(worst, float(e_cal.max()))
        for (name, fr, raw_fr, cal_fr), t in zip(images[1:], FRAMES):
            before, full_b = _cost(lib, capi, b, t, raw_key, raw_fr)
            after, full_a = _cost(lib, capi, b, t, cal_key, cal_fr)
            ideal, _ = _cost(lib, capi, b, t, key, fr)
            print("pair %d %-8s: level-0 cost raw %.1f, calibrated %.2f (the rendered frames themselves: %.2f), full keypoints %d / %d"
                  % (b, name, before, after, ideal, full_b, full_a))
            assert full_b == full_a == sc.entry(b)["K"] and after < before
    print("worst |corrected - scale I| %.2f grey levels (WORST %.2f, tolerance %.2f)" % (worst, WORST, TOL))
    assert worst <= WORST  # (the constant is the measurement)
