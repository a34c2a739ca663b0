"""The caller's points in the raw camera's geometry (mbavo_undistort_points_batch, mbavo_pairs_set_points_geometry): what can be
held without a GPU.  The two entries exist in the library, the header and the binding and return MBAVO_E_ARG before they touch a
device; the numpy restatement of the header's inverse camera (tests/pairs_points_raw_ref.py) agrees with itself point by point and
over arrays, bit for bit; the forward entry of the map restatements, applied to the inverse of every 7th raw pixel of a 640 x 480
image, returns the raw pixel; and hand-made cases give what the header says by hand.

The round trip's bounds are 4 x the restatement's own worst error, measured once and recorded in
profiles/r29_pairs_points_raw.txt: 2.842e-13 px for the radial-tangential camera (a few ulps of a coordinate of some hundred
pixels through the iteration) and 2.143e-05 px for the unified one, where the reference's `float` lambda (24 bits on a
coordinate of up to 640 px) dominates."""
import ctypes as C
import os
import re

import numpy as np

import pairs_api_support as api
import pairs_cameras_ref as cref
import pairs_points_raw_ref as rref
import pairs_undistort_ref as uref
import pairs_unified_ref as xref
import pairs_valid_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_undistort_points_batch", "mbavo_pairs_set_points_geometry"]
E_ARG = -1
HS, WS = 480, 640
# worst |forward(inverse(raw pixel)) - raw pixel| of the restatement over every 7th pixel (profiles/r29_pairs_points_raw.txt)
MEASURED = {1: 2.8421709430404007e-13, 2: 2.1429263256322884e-05}

# a camera and a raw pixel whose iteration has not stopped after 5 steps, frozen from unsolved_search() below: the corner of
# the 60 x 80 radial-tangential camera of the clearance tests, whose distortion folds back before the corner is reached
UNSOLVED_CAMERA, UNSOLVED_PIXEL = "radtan", (0.0, 0.0)
# a unified camera with xi > 1 (no camera of the other tests has one): lambda - xi < 0 from about 20 px off the axis, beta < 0 further out


def round_trip_cameras():
    """One camera of each model at 640 x 480, from the parameter sets of the pairs tests that stay inside the raw image."""
    K = uref.intrinsics(HS, WS)
    s = xref.SETS["inside"]
    return {1: dict(model=1, Hs=HS, Ws=WS, from_intr=K, xi=0.0, dist=uref.DIST_INSIDE, to_intr=K),
            2: dict(model=2, Hs=HS, Ws=WS, from_intr=xref.from_intrinsics("inside", "same", HS, WS), xi=s["xi"], dist=s["dist"], to_intr=K)}


def every_7th_pixel():
    v, u = np.mgrid[0:HS:7, 0:WS:7]
    return np.stack([u.ravel(), v.ravel()], 1).astype(np.float64)


def unsolved_search(name):
    """The first raw pixel, row by row, of a camera of the clearance tests whose iteration takes 5 steps without stopping."""
    cam = vref.CAMERAS[name]
    v, u = np.mgrid[0:cam["Hs"], 0:cam["Ws"]]
    uv = np.stack([u.ravel(), v.ravel()], 1).astype(np.float64)
    _, ok, steps = rref.inverse(cam, uv, want_steps=True)
    i = int(np.flatnonzero((ok == 0) & (steps == rref.STEPS))[0])
    return tuple(uv[i])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert lib.mbavo_abi_version() == 3  # the change only adds
    assert lib.mbavo_pairs_opts_size() == C.sizeof(capi.PairsOpts) == 272 and lib.mbavo_pairs_camera_size() == C.sizeof(capi.PairsCamera) == 120


def test_the_entries_return_e_arg_before_they_touch_a_device(mbavo):
    lib = mbavo.load()
    assert lib.mbavo_undistort_points_batch(None, 1, None, None, None, None, None) == E_ARG
    assert lib.mbavo_pairs_set_points_geometry(None, 0) == E_ARG and lib.mbavo_pairs_set_points_geometry(None, 1) == E_ARG
    from mba_vo_amd import workloads
    assert callable(workloads.PairBatch.set_points_geometry) and callable(workloads.undistort_points_batch)


def test_the_header_no_longer_calls_raw_points_out_of_scope():
    text = open(os.path.join(ROOT, "include", "mbavo.h")).read()
    assert "points given in the raw geometry" not in text and "the points are not raw" not in text
    assert "Out of scope: sub-pixel keypoints, de-duplication." in text


# ---- the two restatements
def test_point_by_point_and_over_arrays_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    cams = list(round_trip_cameras().values()) + list(vref.CAMERAS.values()) + cref.cameras("crop") + [api.XI_ABOVE_1]
    for cam in cams:
        uv = np.stack([rng.uniform(-5, cam["Ws"] + 5, 150), rng.uniform(-5, cam["Hs"] + 5, 150)], 1)
        uv = np.concatenate([np.array(rref.edge_points(cam)), uv])
        xy, ok = rref.inverse(cam, uv)
        one = [rref.inverse_point(cam, u, v) for u, v in uv]
        assert np.array_equal(_bits(xy), _bits([p[:2] for p in one])), cam
        assert ok.tolist() == [int(p[2]) for p in one]
        assert (np.isnan(xy).all(1) == (ok == 0)).all() and np.isfinite(xy[ok == 1]).all()
    # the cameras with a strong lens leave points without a solution, the others none
    assert 0 < rref.inverse(vref.CAMERAS["radtan"], [[1.0, 1.0], [40.0, 30.0]])[1].sum() < 2


def test_the_forward_entry_is_the_map_restatements_entry():
    """rref.forward at whole pixels, converted to float, is the map of the model's restatement."""
    for cam in list(round_trip_cameras().values()) + list(vref.CAMERAS.values()):
        yy, xx = np.mgrid[0:48, 0:64]
        sx, sy = rref.forward(cam, xx.astype(np.float64), yy.astype(np.float64))
        got = np.stack([sx, sy], 2).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), cref.camera_map(cam, 48, 64).view(np.uint32)), cam["model"]


# ---- the round trip
def test_forward_of_inverse_returns_the_raw_pixel():
    uv = every_7th_pixel()
    assert len(uv) == 6348
    for model, cam in round_trip_cameras().items():
        xy, ok, steps = rref.inverse(cam, uv, want_steps=True)
        assert ok.all(), (model, int((ok == 0).sum()))  # a condition on the chosen cameras
        sx, sy = rref.forward(cam, xy[:, 0], xy[:, 1])
        worst = float(max(np.abs(sx - uv[:, 0]).max(), np.abs(sy - uv[:, 1]).max()))
        print("round trip, model %d: worst error %.17g px over %d pixels, at most %d steps (recorded %.17g, bound 4 x)" % (
            model, worst, len(uv), int(steps.max()), MEASURED[model]))
        assert steps.max() <= 4
        assert worst <= 4 * MEASURED[model], (model, worst)
    assert MEASURED[2] > 1e6 * MEASURED[1]  # the float lambda, not the iteration, is model 2's error


# ---- hand-made cases
def test_the_principal_point_maps_to_the_principal_point():
    for cam in list(round_trip_cameras().values()) + list(vref.CAMERAS.values()):
        X, Y, ok = rref.inverse_point(cam, cam["from_intr"][2], cam["from_intr"][3])
        # q = 0 exactly: the first step's error is 0 and the test stops it; x (1 + 1e-8) = 0; lambda (0) = (xi + 1) / 1
        assert ok and (X, Y) == (cam["to_intr"][2], cam["to_intr"][3]), cam
        assert rref.undistort_normalised(cam["dist"], 0.0, 0.0) == (0.0, 0.0, True, 1)


def test_zero_distortion_is_the_affine_change_of_camera():
    cam = dict(model=1, Hs=60, Ws=80, from_intr=(61.0, 59.0, 40.25, 29.5), xi=0.0, dist=uref.DIST_NONE, to_intr=(38.0, 37.5, 31.8, 23.3))
    rng = np.random.default_rng(4)
    uv = np.stack([rng.uniform(0, 79, 200), rng.uniform(0, 59, 200)], 1)
    xy, ok, steps = rref.inverse(cam, uv, want_steps=True)
    fx, fy, cx, cy = cam["from_intr"]
    tfx, tfy, tcx, tcy = cam["to_intr"]
    # the steps still run: d(q) = q, J = I, so e = 0, du = 0 and the first test stops (the second step of the header's wording is
    # the one after a start off the solution; from q = p the start is the solution)
    assert ok.all() and (steps == 1).all()
    want = np.stack([tfx * (((uv[:, 0] - cx) / fx) * (1.0 + 1e-8)) + tcx, tfy * (((uv[:, 1] - cy) / fy) * (1.0 + 1e-8)) + tcy], 1)
    assert np.array_equal(_bits(xy), _bits(want))
    # ... and with the unified model at xi = 0: lambda = (float)((0 + sqrtf(1 + rho2)) / (1 + rho2)), x = lambda q / lambda up to a rounding
    uni = dict(cam, model=2)
    xy2, ok2 = rref.inverse(uni, uv)
    assert ok2.all() and np.abs(xy2 - want).max() < 1e-12


def test_no_number_in_no_number_out():
    nan, inf = float("nan"), float("inf")
    for cam in (vref.CAMERAS["radtan"], vref.CAMERAS["unified"]):
        for bad in (nan, inf, -inf):
            for u, v in ((bad, 30.0), (40.0, bad), (bad, bad)):
                X, Y, ok = rref.inverse_point(cam, u, v)
                assert not ok and np.isnan(X) and np.isnan(Y), (cam["model"], u, v)
        xy, ok = rref.inverse(cam, [[nan, 30.0], [40.0, 30.0], [40.0, -inf]])
        assert ok.tolist() == [0, 1, 0] and np.isnan(xy[[0, 2]]).all() and np.isfinite(xy[1]).all()


def test_an_iteration_that_does_not_stop_has_no_solution():
    assert unsolved_search(UNSOLVED_CAMERA) == UNSOLVED_PIXEL  # (the frozen constants are what the search finds)
    cam = vref.CAMERAS[UNSOLVED_CAMERA]
    fx, fy, cx, cy = cam["from_intr"]
    qx, qy, solved, steps = rref.undistort_normalised(cam["dist"], (UNSOLVED_PIXEL[0] - cx) / fx, (UNSOLVED_PIXEL[1] - cy) / fy)
    assert steps == 5 and not solved and np.isfinite(qx) and np.isfinite(qy)  # the reference would return this q
    X, Y, ok = rref.inverse_point(cam, *UNSOLVED_PIXEL)
    assert not ok and np.isnan(X) and np.isnan(Y)
    xy, okv = rref.inverse(cam, [UNSOLVED_PIXEL, (40.0, 30.0)])
    assert okv.tolist() == [0, 1] and np.isnan(xy[0]).all()


def test_a_unified_camera_with_xi_above_1():
    cam = api.XI_ABOVE_1
    fx, _, cx, cy = cam["from_intr"]
    xi = cam["xi"]

    def parts(u):
        rho2 = np.float32(((u - cx) / fx) ** 2)
        beta = np.float32(1.0 + (1.0 - xi * xi) * np.float64(rho2))
        with np.errstate(invalid="ignore"):
            lam = np.float32((xi + np.float64(np.sqrt(beta))) / (1.0 + np.float64(rho2)))
        return beta, np.float64(lam) - xi

    assert rref.inverse_point(cam, cx, cy) == (cam["to_intr"][2], cam["to_intr"][3], True)
    near = rref.inverse_point(cam, cx + 10.0, cy)
    assert near[2] and near[0] > cam["to_intr"][2] and parts(cx + 10.0)[0] > 0 and parts(cx + 10.0)[1] > 0
    beta, pz = parts(cx + 20.5)  # beta still positive, the ray already behind the camera
    assert beta > 0 and pz < 0 and rref.inverse_point(cam, cx + 20.5, cy)[2] is False
    beta, _ = parts(cx + 39.5)   # the last column: beta < 0
    assert beta < 0
    X, Y, ok = rref.inverse_point(cam, cx + 39.5, cy)
    assert not ok and np.isnan(X) and np.isnan(Y)
    xy, okv = rref.inverse(cam, [[cx + 10.0, cy], [cx + 20.5, cy], [cx + 39.5, cy]])
    assert okv.tolist() == [1, 0, 0] and np.isnan(xy[1:]).all()


def test_the_raw_bounds_test():
    Hs, Ws = 60, 80
    inf = float("inf")
    inside = [(-0.0, -0.0), (0.0, 0.0), (Ws - 1.0, Hs - 1.0), (-0.0, Hs - 1.0), (Ws - 1.0, -0.0), (39.5, 29.25)]
    outside = [(np.nextafter(0.0, -1.0), 5.0), (5.0, np.nextafter(0.0, -1.0)), (np.nextafter(Ws - 1.0, inf), 5.0), (5.0, np.nextafter(Hs - 1.0, inf)),
               (-1.0, 5.0), (float(Ws), 5.0), (5.0, float(Hs)), (float("nan"), 5.0), (5.0, float("nan")), (inf, 5.0), (5.0, -inf)]
    assert rref.raw_inside(inside, Hs, Ws).all() and not rref.raw_inside(outside, Hs, Ws).any()
    # a point outside the raw image has no pixel, whatever the inverse camera would say of it
    cam = vref.CAMERAS["unified"]
    assert rref.inverse_point(cam, -1.0, 30.0)[2] and np.isnan(rref.to_undistorted(cam, [[-1.0, 30.0]])).all()
    got = rref.to_undistorted(cam, inside)
    assert np.array_equal(_bits(got), _bits(rref.inverse(cam, inside)[0])) and np.isfinite(got).all()


def test_the_composition_drops_what_has_no_pixel_and_keeps_the_order():
    cam = vref.CAMERAS["radtan"]
    H, W, L, borders = vref.H, vref.W, vref.L, (3, 2, 1)
    uv = np.array([(40.0, 30.0), UNSOLVED_PIXEL, (-1.0, 30.0), (41.0, 30.0), (float("nan"), 3.0), (39.0, 31.0)])
    z = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    kp, counts = rref.keypoints([(uv, z)], [cam], L, H, W, borders)
    assert counts.tolist() == [[3, 3, 3]] and kp[0]["z"].tolist() == [1.0, 4.0, 6.0]
    X, Y, _ = rref.inverse_point(cam, 40.0, 30.0)
    assert kp[0]["xy"][0].tolist() == [np.floor(X + 0.5), np.floor(Y + 0.5)]
