"""A set of G cameras in one batch of pairs (mbavo_pairs_opts.num_cameras, mbavo_pairs_camera, mbavo_pairs_set_cameras,
mbavo_undistort_map_batch): what can be held without a GPU.  The entry points exist in the library, the header and the binding;
the structs have the sizes of their ctypes mirrors and mbavo_pairs_opts has not grown; mbavo_pairs_plan counts G maps where it
counted one and none with undistort = 0; and the camera set the GPU tests use (tests/pairs_cameras_ref.py) has the witnesses it
is chosen for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_api_support as api
import pairs_cameras_ref as cref
import pairs_undistort_ref as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_pairs_camera_size", "mbavo_pairs_set_cameras", "mbavo_undistort_map_batch"]


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert re.search(r"\bnum_cameras\s*;", header)
    assert lib.mbavo_abi_version() == 3
    # validated before anything touches a device: no context, no object, no call
    cam, idx = capi.PairsCamera(), (C.c_int * 1)(0)
    assert lib.mbavo_pairs_set_cameras(None, 1, C.byref(cam), idx) == api.E_ARG
    assert lib.mbavo_undistort_map_batch(None, 1, C.byref(cam), 48, 64, None) == api.E_ARG


def test_structs_have_the_sizes_and_offsets_of_the_header(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    P, Cam = capi.PairsOpts, capi.PairsCamera
    assert lib.mbavo_pairs_opts_size() == C.sizeof(P) == 272  # unchanged
    assert P.num_cameras.offset == 260 == P.undistort.offset + 4 and P.num_cameras.size == 4
    assert P.reserved.offset == 244 and P.reserved.size == 28  # `reserved` stays the name of the whole tail
    assert lib.mbavo_pairs_camera_size() == C.sizeof(Cam) == 120
    assert (Cam.model.offset, Cam.reserved.offset, Cam.H.offset, Cam.W.offset, Cam.intrinsics.offset, Cam.xi.offset, Cam.dist.offset,
            Cam.to_intrinsics.offset) == (0, 4, 8, 12, 16, 48, 56, 88)
    assert lib.mbavo_camera_radtan_size() == 72 and lib.mbavo_camera_unified_size() == 80
    o = P()
    assert o.num_cameras == 0  # a zeroed struct is today's behaviour
    o.num_cameras = 3
    assert bytes(o)[260:264] == np.array([3], np.int32).tobytes() and list(o.reserved)[4] == 3


def test_workloads_fill_the_struct(mbavo):
    from mba_vo_amd import workloads
    rad = workloads.pairs_camera(workloads.camera_radtan(52, 76, (1.0, 2.0, 3.0, 4.0), (5.0, 6.0, 7.0, 8.0)), (9.0, 10.0, 11.0, 12.0))
    assert isinstance(rad, mbavo.capi.PairsCamera) and (rad.model, rad.reserved, rad.H, rad.W, rad.xi) == (1, 0, 52, 76, 0.0)
    assert list(rad.intrinsics) == [1.0, 2.0, 3.0, 4.0] and list(rad.dist) == [5.0, 6.0, 7.0, 8.0] and list(rad.to_intrinsics) == [9.0, 10.0, 11.0, 12.0]
    uni = workloads.pairs_camera(workloads.camera_unified(50, 70, (1.0, 2.0, 3.0, 4.0), 1.05), (9.0, 10.0, 11.0, 12.0))
    assert (uni.model, uni.H, uni.W, uni.xi) == (2, 50, 70, 1.05) and list(uni.dist) == [0.0] * 4


def _align(v, a=256):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("kw", [dict(), dict(B=3, L=2, H=75, W=101, cell=12), dict(B=64, H=480, W=640, fmt=2), dict(B=4, L=3, H=45, W=63, cell=6)])
def test_plan_counts_one_map_per_camera(mbavo, kw):
    """num_cameras = G costs the num_cameras = 0 plan plus 8 H W (G - 1) bytes after alignment with undistort 1 and 2, and not a
    byte with undistort = 0 (no map at all); nothing else of the plan moves.  num_cameras of -1 or B + 1 is MBAVO_E_ARG."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    B, H, W = kw.get("B", 4), kw.get("H", 120), kw.get("W", 160)
    for u in (0, 1, 2):
        plans = {}
        for G in (0, 1, 2, B):
            o = api.opts(capi, keep=keep, **kw)
            o.undistort, o.num_cameras = u, G
            plans[G] = api.plan(lib, o)
            assert plans[G][0] == 0, (u, G, plans[G])
            assert plans[G][2] == plans[0][2]  # the capacities do not know the cameras
        for G in (1, 2, B):
            want = 0 if u == 0 else _align(8 * H * W * G) - _align(8 * H * W)
            assert plans[G][1] - plans[0][1] == want, (u, G)
        assert plans[1][1] == plans[0][1]
    for bad in (-1, B + 1, 1 << 30, -(1 << 31)):
        for u in (0, 1):
            o = api.opts(capi, keep=keep, **kw)
            o.undistort, o.num_cameras = u, bad
            rc, nbytes, _ = api.plan(lib, o)
            assert rc == api.E_ARG and nbytes == -7, (bad, u)


@pytest.mark.parametrize("geometry", list(cref.GEOMETRIES))
def test_the_camera_set_has_its_witnesses(geometry):
    """Camera 0 points 1 % .. 10 % of the pixels at a tap outside the raw image, camera 1 none; the three to_intrinsics differ
    in all four entries, pairwise; two pairs share camera 0 and the index pattern does not ascend; the three maps differ."""
    H, W, Hs, Ws = cref.GEOMETRIES[geometry]
    cams = cref.cameras(geometry)
    maps = cref.maps_of(cams, H, W)
    assert maps.shape == (3, H, W, 2) and maps.dtype == np.float32
    share = uref.tap_outside(maps[0], Hs, Ws).mean()
    print("share of pixels with a tap outside, camera 0, %s: %.4f" % (geometry, share))
    assert 0.01 < share < 0.10
    assert not uref.tap_outside(maps[1], Hs, Ws).any()
    assert [c["model"] for c in cams] == [1, 2, 1] and not any(cams[2]["dist"]) and cams[1]["xi"] > 0
    for i in range(3):
        for j in range(i + 1, 3):
            assert all(a != b for a, b in zip(cams[i]["to_intr"], cams[j]["to_intr"])), (i, j)
            assert np.abs(maps[i] - maps[j]).max() > 1.0
    idx = cref.CAMERA_OF_PAIR
    assert sorted(set(idx)) == [0, 1, 2] and idx.count(0) == 2 and list(idx) != sorted(idx)
    assert sorted(cref.SWAPPED) == sorted(idx) and [b for b in range(4) if cref.SWAPPED[b] != idx[b]] == [1, 3]
    assert (H * W) % 2 == (1 if geometry == "odd" else 0)  # "odd": maps 1 (and the images through it) start off a 16-byte boundary
    per_pair = cref.per_pair(maps, idx)
    assert per_pair.shape == (4, H, W, 2) and np.array_equal(per_pair[0], per_pair[2]) and np.array_equal(per_pair[3], maps[2])
    K = cref.level_intrinsics(cams, idx, 3)
    assert K.shape == (4, 3, 4) and np.array_equal(K[1, 2], np.array(cams[1]["to_intr"]) / 4.0)
