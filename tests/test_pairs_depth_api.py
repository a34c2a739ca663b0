"""Depth formats of mbavo_pairs (mbavo_pairs_opts.depth_format, depth_unit, depth_max) and mbavo_depth_to_z: what can be held
without a GPU.  The entry point exists in the library, the header and the binding; mbavo_pairs_plan accepts formats 0, 1, 2 with
one byte count and rejects everything else; the options struct has the size it had; and the numpy restatement the GPU tests use
as their expectation (tests/pairs_depth_ref.py) gives, at the edges of the depth test, the values include/mbavo.h's formulas
give when worked by hand."""
import ctypes as C
import os
import re

import numpy as np

import pairs_api_support as api
import pairs_depth_ref as zref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = (90.0, 90.0, 50.0, 37.0)  # fx, fy, cx, cy on a 75 x 101 map


def _depth_opts(capi, keep, depth_format=0, unit=0.0, dmax=0.0, **kw):
    o = api.opts(capi, keep=keep, **kw)
    o.depth_format, o.depth_unit, o.depth_max = depth_format, unit, dmax
    return o


def test_entry_point_is_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    assert hasattr(C.CDLL(mbavo.LIB_PATH), "mbavo_depth_to_z")
    assert re.search(r"\bmbavo_depth_to_z\s*\(", header) and "mbavo_depth_to_z" in capi.SYMBOLS
    for field in ("depth_format", "depth_unit", "depth_max"):
        assert re.search(r"\b%s\s*;" % field, header), field
    # validated before anything touches a device: no context, no call
    K = (C.c_double * 4)(*INTR)
    assert lib.mbavo_depth_to_z(None, 1, None, 4, 4, K, 0.0, 0.0, None) == api.E_ARG


def test_options_struct_keeps_its_size(mbavo):
    """272 bytes, as before the fields were taken from `reserved`; they follow every_candidate; a zeroed struct is format 0."""
    lib, capi = mbavo.load(), mbavo.capi
    P = capi.PairsOpts
    assert lib.mbavo_pairs_opts_size() == C.sizeof(P) == 272
    assert P.depth_format.offset == P.every_candidate.offset + 4 == 244
    assert (P.depth_unit.offset, P.depth_max.offset) == (248, 252) and P.depth_max.offset + 4 + 4 * 4 == 272
    o = P()
    assert (o.depth_format, o.depth_unit, o.depth_max) == (0, 0.0, 0.0)
    o.depth_format, o.depth_unit, o.depth_max = 2, 5000.0, 100.0
    raw = bytes(o)[244:256]
    assert raw == np.array([2], np.int32).tobytes() + np.array([5000.0, 100.0], np.float32).tobytes()


def test_plan_accepts_the_three_formats_with_one_byte_count(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for kw in (dict(), dict(B=3, L=2, H=75, W=101, cell=12, fmt_kf=1), dict(B=64, H=480, W=640, fmt_kf=2)):
        kf = kw.pop("fmt_kf", 0)
        plans = [api.plan(lib, _depth_opts(capi, keep, f, unit, dmax, fmt=kf, **kw)) for f, unit, dmax in
                 ((0, 0.0, 0.0), (1, 0.0, 0.0), (1, 0.0, 100.0), (2, 5000.0, 0.0), (2, 1e-3, 7.0), (0, -1.0, -1.0), (1, -5.0, -1.0))]
        assert all(p[0] == 0 for p in plans), plans
        assert len({(p[1], tuple(p[2])) for p in plans}) == 1 and plans[0][1] > 0  # the object stores no depth map
    # every_candidate as well
    o = _depth_opts(capi, keep, 2, 5000.0, cell=0)
    o.every_candidate = 1
    z = _depth_opts(capi, keep, 0, cell=0)
    z.every_candidate = 1
    assert api.plan(lib, o) == api.plan(lib, z) and api.plan(lib, o)[0] == 0


def test_plan_rejects_other_formats_and_units(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for depth_format, unit in ((3, 5000.0), (-1, 5000.0), (2, 0.0), (2, -5000.0), (2, float("nan")), (7, 0.0)):
        for every in (0, 1):
            o = _depth_opts(capi, keep, depth_format, unit)
            o.every_candidate = every
            rc, nb, _ = api.plan(lib, o)
            assert rc == api.E_ARG and nb == -7, (depth_format, unit, every)  # (nothing written on an error)
    # create validates before it looks at the context
    h = C.c_void_p()
    assert lib.mbavo_pairs_create(None, C.byref(_depth_opts(capi, keep, 3)), C.byref(h)) == api.E_ARG and not h.value


def test_uint16_edges():
    """unit 5000: 50 -> float32(0.01), whose double lies below 1e-2: dropped; 51 kept; 0 dropped."""
    z = zref.u16_to_z(np.array([[50, 51, 0, 65535, 5000]], np.uint16), 5000.0)
    assert z[0, 0] == np.float32(0.01) and float(z[0, 0]) < 1e-2
    assert zref.has_depth(z).tolist() == [[False, True, False, True, True]]
    assert z[0, 4] == 1.0 and z[0, 3] == np.float32(65535 / 5000.0) and z[0, 2] == 0.0
    # the division is done in double and rounded once
    v = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    assert np.array_equal(zref.u16_to_z(v, 5000.0), np.array([np.float32(int(i) / 5000.0) for i in v.ravel()]).reshape(256, 256))
    assert zref.to_z(2, v[None], INTR, 5000.0).shape == (1, 256, 256)


def _ray_at(d, x, y, dmax=0.0, H=75, W=101):
    m = np.ones((H, W), np.float32)
    m[y, x] = np.float32(d)
    return zref.ray_to_z(m, INTR, dmax)[y, x]


def test_ray_distance_edges():
    """fx = fy = 90, cx = 50, cy = 37 on a 75 x 101 map."""
    # by hand at pixel (0, 0): xn = -50 / 90, yn = -37 / 90
    xn, yn = (0.0 - 50.0) / 90.0, (0.0 - 37.0) / 90.0
    n = np.sqrt(xn * xn + yn * yn + 1.0)
    z = _ray_at(0.0125, 0, 0)
    assert z == np.float32(np.float64(np.float32(0.0125)) * (1.0 / n))
    assert abs(float(z) - 0.010283089) < 5e-10 and zref.has_depth(z)
    z = _ray_at(0.0102, 0, 0)
    assert abs(float(z) - 0.0084) < 5e-5 and not zref.has_depth(z)
    assert zref.has_depth(np.float32(0.0102))  # format 0 would keep the same number
    # at the principal point n = 1: z = d
    d = np.float32(0.01)
    up = np.nextafter(d, np.float32(1))
    assert _ray_at(d, 50, 37) == d and not zref.has_depth(_ray_at(d, 50, 37))
    assert _ray_at(up, 50, 37) == up and zref.has_depth(_ray_at(up, 50, 37))
    # depth_max = 100: 100.0 converts normally, the next float above it is no depth; without a limit it converts
    hundred = np.float32(100)
    above = np.nextafter(hundred, np.float32(200))
    assert _ray_at(hundred, 50, 37, 100.0) == hundred and _ray_at(above, 50, 37, 100.0) == 0.0
    assert _ray_at(above, 50, 37, 0.0) == above and _ray_at(above, 50, 37, -1.0) == above
    far = _ray_at(hundred, 100, 74, 100.0)  # the last row and column
    assert 0 < far < hundred and far == np.float32(100.0 * (1.0 / np.sqrt((50.0 / 90.0) ** 2 + (37.0 / 90.0) ** 2 + 1.0)))
    # z never exceeds the distance
    rng = np.random.default_rng(0)
    m = rng.uniform(0, 120, (75, 101)).astype(np.float32)
    zz = zref.ray_to_z(m, INTR, 100.0)
    assert np.all(zz <= m) and np.all(zz[m > 100] == 0) and np.all(zz[(m <= 100) & (m > 0)] > 0)
    assert np.array_equal(zref.to_z(1, m, INTR, 0.0, 100.0), zz) and np.array_equal(zref.to_z(0, m, INTR), m)


def test_python_wrapper_checks_dtypes(mbavo):
    import torch
    from mba_vo_amd import workloads
    assert workloads.depth_dtypes(0) == (torch.float32,) == workloads.depth_dtypes(1)
    assert torch.float32 not in workloads.depth_dtypes(2) and len(workloads.depth_dtypes(2)) >= 1
    assert all(torch.empty(0, dtype=d).element_size() == 2 for d in workloads.depth_dtypes(2))
