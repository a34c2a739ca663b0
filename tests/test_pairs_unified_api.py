"""The unified camera (mbavo_camera_unified, mbavo_undistort_map_unified, mbavo_pairs_set_camera_unified) and the batched remap
(mbavo_undistort_u8_batch): what can be held without a GPU.  The entry points exist in the library, the header and the binding,
and the ABI numbers have not moved.  The model of the numpy restatement the GPU tests use as their expectation
(tests/pairs_unified_ref.py) is pinned independently of the code under test: the reference's own inverse of the projection,
CameraUnified::unproject with its `float` temporaries, restated here, returns the ray each map entry was projected from.  The
xi = 0 map is the closed-form affine grid bit for bit, and the parameter sets have the witnesses they are chosen for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_undistort_ref as uref
import pairs_unified_ref as xref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ["mbavo_camera_unified_size", "mbavo_undistort_map_unified", "mbavo_undistort_u8_batch", "mbavo_pairs_set_camera_unified"]
GEOMETRIES = {"crop": (48, 64, 52, 76), "same": (50, 70, 50, 70)}  # H, W of the undistorted camera, Hs, Ws of the raw one
CASES = [(g, s) for g in GEOMETRIES for s in xref.SETS]


def _maps(geometry, name, dtype=np.float32):
    H, W, Hs, Ws = GEOMETRIES[geometry]
    s = xref.SETS[name]
    from_intr, to_intr = xref.from_intrinsics(name, geometry, Hs, Ws), xref.intrinsics(H, W)
    return xref.undistort_map(from_intr, s["xi"], s["dist"], to_intr, H, W, dtype=dtype), from_intr, to_intr


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    # validated before anything touches a device: no context, no object, no call
    cam = capi.CameraUnified()
    K = (C.c_double * 4)(100.0, 100.0, 32.0, 24.0)
    assert lib.mbavo_undistort_map_unified(None, C.byref(cam), K, 48, 64, None) == E_ARG
    assert lib.mbavo_undistort_u8_batch(None, None, 1, 48, 64, None, 48, 64, None) == E_ARG
    assert lib.mbavo_pairs_set_camera_unified(None, C.byref(cam)) == E_ARG


def test_sizes_and_abi_have_not_moved(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    Cam = capi.CameraUnified
    assert lib.mbavo_camera_unified_size() == C.sizeof(Cam) == 80
    assert (Cam.H.offset, Cam.W.offset, Cam.intrinsics.offset, Cam.xi.offset, Cam.dist.offset) == (0, 4, 8, 40, 48)
    assert lib.mbavo_abi_version() == 3
    assert lib.mbavo_pairs_opts_size() == C.sizeof(capi.PairsOpts) == 272
    assert lib.mbavo_camera_radtan_size() == C.sizeof(capi.CameraRadTan) == 72


def test_workloads_fill_the_struct(mbavo):
    from mba_vo_amd import workloads
    cam = workloads.camera_unified(52, 76, (1.0, 2.0, 3.0, 4.0), 1.05, (5.0, 6.0, 7.0, 8.0))
    assert isinstance(cam, mbavo.capi.CameraUnified) and (cam.H, cam.W, cam.xi) == (52, 76, 1.05)
    assert list(cam.intrinsics) == [1.0, 2.0, 3.0, 4.0] and list(cam.dist) == [5.0, 6.0, 7.0, 8.0]
    assert list(workloads.camera_unified(1, 1, (1, 1, 0, 0), 0.0).dist) == [0.0] * 4


# ---- the reference's own inverse, restated: DistortionRadTan::undistort (five Gauss-Newton steps on `distort`, each with its
# Jacobian) and CameraUnified::unproject, whose rho2_u, beta and lambda are `float` variables.
def _distort_with_jacobian(k1, k2, p1, p2, x, y):
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    dx = x + x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
    dy = y + y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
    j00 = 1.0 + rad + 2.0 * k1 * mx2 + 4.0 * k2 * mx2 * rho2 + 2.0 * p1 * y + 6.0 * p2 * x
    j01 = 2.0 * k1 * mxy + 4.0 * k2 * rho2 * mxy + 2.0 * p1 * x + 2.0 * p2 * y
    j11 = 1.0 + rad + 2.0 * k1 * my2 + 4.0 * k2 * my2 * rho2 + 2.0 * p2 * x + 6.0 * p1 * y
    return dx, dy, j00, j01, j11


def _radtan_undistort(dist, px, py):
    """Five steps for every point (the reference stops a point early once its residual is below 1e-15 squared; a step more from
    there moves it by less than that)."""
    x, y = px.copy(), py.copy()
    for _ in range(5):
        dx, dy, j00, j01, j11 = _distort_with_jacobian(*dist, x, y)
        ex, ey = px - dx, py - dy
        det = j00 * j11 - j01 * j01  # (J is symmetric and square: (J^T J)^-1 J^T e = J^-1 e)
        x, y = x + (j11 * ex - j01 * ey) / det, y + (j00 * ey - j01 * ex) / det
    return x, y


def _unified_unproject(from_intr, xi, dist, p2d):
    """(ok, H x W x 3 point at z = 1) of double pixel positions p2d."""
    fx, fy, cx, cy = (np.float64(v) for v in from_intr)
    x, y = (p2d[..., 0] - cx) / fx, (p2d[..., 1] - cy) / fy
    if any(dist):
        x, y = _radtan_undistort([np.float64(v) for v in dist], x, y)
    rho2 = (x * x + y * y).astype(np.float32)
    beta = (1.0 - np.float64(xi) * xi) * rho2.astype(np.float64)
    beta = (1.0 + beta).astype(np.float32)
    lam = ((xi + np.sqrt(beta.astype(np.float64))) / (1.0 + rho2.astype(np.float64))).astype(np.float32).astype(np.float64)
    P = np.stack([lam * x, lam * y, lam - xi], -1)
    ok = (beta >= 0) & (P[..., 2] >= 0)
    return ok, P / P[..., 2:3], (x, y)


@pytest.mark.parametrize("geometry,name", CASES)
def test_the_reference_s_unproject_returns_the_rays_the_map_projects(geometry, name):
    """unproject(project(P)) = P / P.z for P = (xn, yn, 1) over the whole `to` grid.  Tolerance, first order in u = 2^-24 (one
    rounding to float is at most u relative): the only rounded quantities are rho2_u, beta and lambda.
      lambda = (xi + sqrt(beta)) / (1 + rho2): its own rounding u; through sqrt(beta), beta's rounding at most u / 2; through
      rho2 at most u (rho2 / (1 + rho2) + |1 - xi^2| rho2 / (2 beta)) <= u (0.5 + 0.57) for rho2 < 1, |1 - xi^2| <= 1 and
      beta >= 0.89 (all asserted).  Together: |d lambda / lambda| <= 2.57 u.
      The returned x = lambda x_n / (lambda - xi), everything after lambda in double.  d ln x / d ln lambda = -xi / (lambda - xi),
      and the exact lambda - xi is the z of the unit ray, 1 / d with d = |(xn, yn, 1)|: a factor xi d.
    So |x - xn| <= 2.57 u xi d |xn|, likewise y; z is 1 exactly.  On top 1e-12 absolute for everything double: the inverse of the
    distortion converges quadratically and is asserted below to 1e-13, the rest is a few 2^-53.  With xi = 0 lambda cancels and
    the bound is that 1e-12 alone."""
    H, W, Hs, Ws = GEOMETRIES[geometry]
    s = xref.SETS[name]
    xi = s["xi"]
    m64, from_intr, to_intr = _maps(geometry, name, np.float64)
    ok, P, (x, y) = _unified_unproject(from_intr, xi, s["dist"], m64)
    assert ok.all()
    c, r = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    xn, yn = np.broadcast_to((c - to_intr[2]) / to_intr[0], (H, W)), np.broadcast_to((r - to_intr[3]) / to_intr[1], (H, W))
    d = np.sqrt(xn * xn + yn * yn + 1.0)
    # the premises of the derivation
    rho2 = x * x + y * y
    assert rho2.max() < 1.0 and abs(1.0 - xi * xi) <= 1.0 and (1.0 + (1.0 - xi * xi) * rho2).min() >= 0.89
    dx, dy = _distort_with_jacobian(*[np.float64(v) for v in s["dist"]], x, y)[:2]
    back = np.stack([dx * from_intr[0] + from_intr[2], dy * from_intr[1] + from_intr[3]], -1)
    assert np.abs(back - m64).max() < 1e-13 * max(from_intr[:2])  # the inverse of the distortion has converged
    assert np.abs(x - xn / (1.0 + xi * d)).max() < 1e-13
    u = 2.0 ** -24
    for got, want in ((P[..., 0], xn), (P[..., 1], yn)):
        tol = 2.57 * u * xi * d * np.abs(want) + 1e-12
        err = np.abs(got - want)
        print("%s %s: max |error| %.3e, max error / tolerance %.3f" % (geometry, name, err.max(), (err / tol).max()))
        assert (err <= tol).all()
    assert np.all(P[..., 2] == 1.0)
    if xi > 0:  # the float temporaries are in play: the error is far above double roundoff, so the bound is no empty statement
        assert np.abs(P[..., 0] - xn).max() > 1e-10


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_xi_zero_is_the_affine_grid_bit_for_bit(geometry):
    """No 1 + 1e-8 in the unified projection: rz = 1.0 / (1.0 + 0.0 * d) = 1, the zero coefficients add exact zeros.  The radtan
    route with zero coefficients does differ from that grid."""
    H, W, Hs, Ws = GEOMETRIES[geometry]
    m, from_intr, to_intr = _maps(geometry, "pinhole")
    grid = xref.affine_grid(from_intr, to_intr, H, W)
    assert m.dtype == np.float32 and m.shape == (H, W, 2) and np.array_equal(m.view(np.uint32), grid.view(np.uint32))
    radtan = uref.undistort_map(from_intr, uref.DIST_NONE, to_intr, H, W)
    assert not np.array_equal(radtan.view(np.uint32), grid.view(np.uint32))
    if geometry == "same":  # the same camera on both sides: the pixel grid itself up to the rounding of (c - cx) / fx * fx + cx
        px = np.stack(np.broadcast_arrays(np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]), 2)
        assert np.abs(m.astype(np.float64) - px).max() < 1e-5


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_parameter_sets_have_their_witnesses(geometry):
    """`outside` points 1 % .. 10 % of the pixels at a tap outside the raw image, `inside` none; both are distortions."""
    H, W, Hs, Ws = GEOMETRIES[geometry]
    out = uref.tap_outside(_maps(geometry, "outside")[0], Hs, Ws)
    print("share of pixels with a tap outside, %s: %.4f" % (geometry, out.mean()))
    assert 0.01 < out.mean() < 0.10
    assert out[0, 0] and out[0, -1] and out[-1, 0] and out[-1, -1] and not out[H // 4:-(H // 4), W // 4:-(W // 4)].any()  # the corners, not the middle
    m, from_intr, to_intr = _maps(geometry, "inside")
    assert not uref.tap_outside(m, Hs, Ws).any()
    for name in ("outside", "inside"):  # more than a pixel away from the affine change of camera with the same focal length
        m, from_intr, to_intr = _maps(geometry, name)
        assert np.abs(m - xref.affine_grid(from_intr, to_intr, H, W)).max() > 1.0
        assert xref.SETS[name]["xi"] > 0 and any(xref.SETS[name]["dist"])
    assert 0.9 < xref.SETS["outside"]["xi"] < 1.1
