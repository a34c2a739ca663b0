"""Undistortion on the device: mbavo_undistort_map, mbavo_undistort_u8 and the pairs batch on raw camera images
(mbavo_pairs_opts.undistort, mbavo_pairs_set_camera).

The stand-alone entry points are held bit for bit to the numpy restatement of include/mbavo.h's formulas
(tests/pairs_undistort_ref.py).  The batch has two routes to the same arrays: the fused one (an undistort = 1 object remaps the raw
images where it would copy them) and the per-image one (mbavo_undistort_u8 over every image, then an undistort = 0 object); every
array of the two objects is compared bit for bit after a prepare, an update and a mbavo_pairs_track_frame.  undistort = 2 (depth
maps in the raw geometry) is held to the restatement's look-up.  Launches, synchronisations and D2H bytes are the documented ones.

Shapes: 48 x 64 from a 52 x 76 raw camera, and 50 x 70 from 50 x 70 (an odd pixel count: the ragged end of four pixels per lane);
L <= 3, B <= 3.  Three coefficient sets: one that points at taps outside the raw image, one that stays inside, and none; every
test asserts the witness it relies on."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_cases as cases
import pairs_depth_ref as zref
import pairs_device as dv
import pairs_step as ps
import pairs_undistort_ref as uref

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.mark.parametrize("shape", ["crop", "same"])
@pytest.mark.parametrize("dist", ["outside", "inside", "none"])
def test_map_equals_numpy_bit_for_bit(mbavo, gpu_ctx, shape, dist):
    """Check 1: every entry of the map, the last (odd) pixel included; also into a buffer that is only 8-byte aligned."""
    import torch
    from mba_vo_amd import workloads
    c = cases.undistort_case(shape, dist)
    cases.witness(c)
    H, W = c["H"], c["W"]
    got = workloads.undistort_map(gpu_ctx, cases.undistort_camera(c), c["intr"], H, W).cpu().numpy()
    assert got.dtype == np.float32 and dv.same_bits(got, c["map"])
    buf = torch.full((2 * H * W + 4,), -7.0, dtype=torch.float32, device="cuda:0")
    K = np.ascontiguousarray(c["intr"], np.float64)
    cam = cases.undistort_camera(c)
    assert gpu_ctx.lib.mbavo_undistort_map(gpu_ctx.handle, C.byref(cam), mbavo.capi.dp(K), H, W, buf.data_ptr() + 8) == 0
    out = buf.cpu().numpy()
    assert dv.same_bits(out[2:-2].reshape(H, W, 2), c["map"]) and np.all(out[:2] == -7.0) and np.all(out[-2:] == -7.0)


@pytest.mark.parametrize("shape", ["crop", "same"])
def test_remap_equals_numpy_byte_for_byte(mbavo, gpu_ctx, shape):
    """Check 2: the distorting map with a NaN, an infinity, entries at 2^31 and 2^30, at -0.5, Ws - 0.5 and Hs - 1; a stack of images;
    and the byte-wise path (a destination and a map that are not aligned)."""
    import torch
    from mba_vo_amd import workloads
    c = cases.undistort_case(shape, "outside")
    assert 0.01 < cases.witness(c) < 0.10
    H, W, Hs, Ws = c["H"], c["W"], c["Hs"], c["Ws"]
    m = cases.special_map(c)
    want = np.stack([uref.remap_u8(im, m) for im in c["raw"]["sharp"]])
    assert (want[:, c["outside"]] == 0).any() and want.max() > 100  # the border rule is in play
    raw_t, map_t = dv.dev(c["raw"]["sharp"], m)
    got = workloads.undistort_u8(gpu_ctx, raw_t, map_t).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # one byte / one float off alignment: the same bytes, and nothing written outside the H * W bytes
    src = torch.zeros(Hs * Ws + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = raw_t[1].view(-1)
    mbuf = torch.zeros(2 * H * W + 1, dtype=torch.float32, device="cuda:0")
    mbuf[1:] = map_t.view(-1)
    dst = torch.full((H * W + 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert gpu_ctx.lib.mbavo_undistort_u8(gpu_ctx.handle, src.data_ptr() + 1, Hs, Ws, mbuf.data_ptr() + 4, H, W, dst.data_ptr() + 3) == 0
    out = dst.cpu().numpy()
    assert np.array_equal(out[3:3 + H * W].reshape(H, W), want[1]) and np.all(out[:3] == 0xA5) and np.all(out[3 + H * W:] == 0xA5)


def test_stand_alone_calls_reject_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    import torch
    from mba_vo_amd import workloads
    lib, capi, c = gpu_ctx.lib, mbavo.capi, cases.undistort_case("crop", "inside")
    H, W, Hs, Ws = c["H"], c["W"], c["Hs"], c["Ws"]
    K = np.ascontiguousarray(c["intr"], np.float64)
    out = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda:0")
    good = cases.undistort_camera(c)

    def cam(**kw):
        k = workloads.camera_radtan(kw.get("H", Hs), kw.get("W", Ws), c["from_intr"], cases.DISTS["inside"])
        for i in kw.get("zero", ()):
            k.intrinsics[i] = 0.0
        return k

    call = lambda k, to, h, w, o: lib.mbavo_undistort_map(gpu_ctx.handle, C.byref(k) if k is not None else None, capi.dp(to) if to is not None else None, h, w, o)
    K0, K1 = K.copy(), K.copy()
    K0[0], K1[1] = 0.0, 0.0
    o = out.data_ptr()
    for args in ((None, K, H, W, o), (good, None, H, W, o), (good, K, H, W, None), (good, K, 0, W, o), (good, K, H, -1, o), (good, K, 2048, 2049, o),
                 (cam(H=0), K, H, W, o), (cam(W=0), K, H, W, o), (cam(H=4096, W=1025), K, H, W, o), (cam(zero=(0,)), K, H, W, o),
                 (cam(zero=(1,)), K, H, W, o), (good, K0, H, W, o), (good, K1, H, W, o)):
        assert call(*args) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    src, dst = torch.zeros((Hs, Ws), dtype=torch.uint8, device="cuda:0"), torch.full((H, W), 0xA5, dtype=torch.uint8, device="cuda:0")
    s, m, d = src.data_ptr(), out.data_ptr(), dst.data_ptr()
    for args in ((None, Hs, Ws, m, H, W, d), (s, Hs, Ws, None, H, W, d), (s, Hs, Ws, m, H, W, None), (s, 0, Ws, m, H, W, d), (s, Hs, Ws, m, H, 0, d),
                 (s, 4096, 1025, m, H, W, d), (s, Hs, Ws, m, 2049, 2048, d)):
        assert lib.mbavo_undistort_u8(gpu_ctx.handle, *args) == E_ARG
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    assert call(good, K, H, W, o) == 0  # and with good arguments it writes
    torch.cuda.synchronize()
    assert dv.same_bits(out.cpu().numpy(), c["map"])


@pytest.mark.parametrize("shape,dist", [("crop", "outside"), ("crop", "inside"), ("same", "outside")])
@pytest.mark.parametrize("kf", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_prepare_on_raw_images_equals_prepare_on_remapped_images(mbavo, gpu_ctx, shape, dist, kf, dense):
    """Check 3: B = 3, L = 3: every image level, gradient image (or packed word), keypoint, depth and count of the undistort = 1
    object equals the undistort = 0 object's on the images mbavo_undistort_u8 gives -- which are the numpy ones."""
    from mba_vo_amd import workloads
    c = cases.undistort_case(shape, dist)
    cases.witness(c)
    raw_s, raw_b, z = dv.dev(c["raw"]["sharp"], c["raw"]["blur"], c["z"])
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense, kf), cases.undistort_batch(gpu_ctx, c, 0, dense, kf)
    try:
        assert fused.set_camera(cases.undistort_camera(c)) == 0
        map_t = workloads.undistort_map(gpu_ctx, cases.undistort_camera(c), c["intr"], c["H"], c["W"])
        und_s, und_b = workloads.undistort_u8(gpu_ctx, raw_s, map_t), workloads.undistort_u8(gpu_ctx, raw_b, map_t)
        assert np.array_equal(und_s.cpu().numpy(), c["und"]["sharp"]) and np.array_equal(und_b.cpu().numpy(), c["und"]["blur"])
        cf, ct = fused.prepare(raw_s, z, raw_b), twin.prepare(und_s, z, und_b)
        assert np.array_equal(cf, ct) and cf.min() > 0
        got = dv.read_batch(fused, cf)
        dv.assert_twins(got, dv.read_batch(twin, ct), (shape, dist, kf, dense))
        for b in range(c["B"]):  # level 0 is the remapped image, the current frame too
            assert np.array_equal(got[b * c["L"]]["ref"], c["und"]["sharp"][b].ravel()) and np.array_equal(got[b * c["L"]]["cur"], c["und"]["blur"][b].ravel())
        assert fused.stats()[3] - twin.stats()[3] >= 8 * c["H"] * c["W"]
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("dense", [False, True])
def test_no_distortion_and_the_same_camera_is_the_plain_prepare(mbavo, gpu_ctx, dense):
    """Check 4: zero coefficients, equal camera, equal size (50 x 70): the undistort = 1 object equals an undistort = 0 object given
    the raw images -- although the 1 + 1e-8 of `project` keeps map entries off the pixel grid."""
    c = cases.undistort_case("same", "none")
    grid = np.stack(np.broadcast_arrays(np.arange(c["W"], dtype=np.float32)[None, :], np.arange(c["H"], dtype=np.float32)[:, None]), 2)
    assert 0.05 < (c["map"] != grid).mean() < 1 and np.array_equal(c["und"]["sharp"], c["raw"]["sharp"])  # (float keeps a tenth of the entries off it)
    raw_s, raw_b, z = dv.dev(c["raw"]["sharp"], c["raw"]["blur"], c["z"])
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense), cases.undistort_batch(gpu_ctx, c, 0, dense)
    try:
        assert fused.set_camera(cases.undistort_camera(c)) == 0
        cf, ct = fused.prepare(raw_s, z, raw_b), twin.prepare(raw_s, z, raw_b)
        assert np.array_equal(cf, ct) and cf.min() > 0
        dv.assert_twins(dv.read_batch(fused, cf), dv.read_batch(twin, ct), ("identity", dense))
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("mode", ["keys and blur", "keys only", "blur only", "second camera"])
@pytest.mark.parametrize("dense", [False, True])
def test_update_equals_a_fresh_prepare_of_the_composite_inputs(mbavo, gpu_ctx, mode, dense):
    """Check 5: key list [0, 2] of B = 3 with and without d_blur, n_key = 0 with a d_blur, and an update after a second set_camera
    with other coefficients (the images it brings go through the new map, pair 1's keyframe keeps the old one).  The expectation
    is an undistort = 0 object prepared on the composite of the remapped images."""
    c, c2 = cases.undistort_case("crop", "outside"), cases.undistort_case("crop", "inside")
    cases.witness(c), cases.witness(c2)
    B, keys = c["B"], ([] if mode == "blur only" else [0, 2])
    with_blur = mode != "keys only"
    new = c2 if mode == "second camera" else c  # (the same raw images in both cases: only the map differs)
    assert np.array_equal(c["raw"]["new_sharp"], c2["raw"]["new_sharp"]) and not np.array_equal(c["und"]["new_sharp"], c2["und"]["new_sharp"])
    sharp, depth = c["und"]["sharp"].copy(), c["z"].copy()
    sharp[keys], depth[keys] = new["und"]["new_sharp"][keys], c["new_z"][keys]
    blur = new["und"]["new_blur"] if with_blur else c["und"]["blur"]
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense), cases.undistort_batch(gpu_ctx, c, 0, dense)
    try:
        assert fused.set_camera(cases.undistort_camera(c)) == 0
        before = fused.prepare(*dv.dev(c["raw"]["sharp"], c["z"], c["raw"]["blur"]))
        if mode == "second camera":
            assert fused.set_camera(cases.undistort_camera(c2)) == 0
        args = [dv.dev(c["raw"]["new_blur"])[0] if with_blur else None, keys]
        if keys:
            args += dv.dev(np.ascontiguousarray(c["raw"]["new_sharp"][keys]), np.ascontiguousarray(c["new_z"][keys]))
        cf = fused.update(*args)
        ct = twin.prepare(*dv.dev(np.ascontiguousarray(sharp), np.ascontiguousarray(depth), np.ascontiguousarray(blur)))
        assert np.array_equal(cf, ct) and np.array_equal(cf[1], before[1]) and (not keys or not np.array_equal(cf[keys], before[keys]))
        got = dv.read_batch(fused, cf)
        dv.assert_twins(got, dv.read_batch(twin, ct), (mode, dense))
        assert np.array_equal(got[c["L"]]["ref"], c["und"]["sharp"][1].ravel())  # pair 1's keyframe: the first camera's
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_raw_geometry_depth_maps_are_looked_up_through_the_map(mbavo, gpu_ctx, fmt, dense):
    """Check 6: undistort = 2 with depth formats 0, 1 and 2, no border margin.  Kept keypoints and their z equal the restatement
    (the raw element nearest to the map entry of the keypoint's level-0 pixel, format 1 with that pixel's ray).  The coefficient
    set points level-0 pixels up to three rows outside the raw map; keypoints there are dropped: with a depth of 1 m at those
    pixels instead, the restatement keeps more."""
    c = cases.undistort_case("wide", "outside")
    cases.witness(c)
    B, o, borders = c["B"], cases.DEPTH_FORMATS[fmt], (0, 0, 0)
    raw_d = cases.raw_depth(fmt, B, c["Hs"], c["Ws"], seed=31 + fmt)
    inside = uref.nearest_raw(c["map"], c["Hs"], c["Ws"])[0]
    z = np.stack([uref.depth_through_map(fmt, raw_d[b], c["map"], c["intr"], o["depth_unit"], o["depth_max"]) for b in range(B)])
    assert (~inside).mean() > 0.03 and np.all(z[:, ~inside] == 0) and 0.7 < zref.has_depth(z[:, inside]).mean() < 0.9
    pb = cases.undistort_batch(gpu_ctx, c, 2, dense, depth=fmt, borders=borders)
    try:
        assert pb.set_camera(cases.undistort_camera(c)) == 0
        counts = pb.prepare(dv.dev(c["raw"]["sharp"])[0], dv.dev_depth(raw_d), dv.dev(c["raw"]["blur"])[0])
        got = dv.read_batch(pb, counts)
        assert counts.min() > 0
        for b in range(B):
            assert np.array_equal(got[b * c["L"]]["ref"], c["und"]["sharp"][b].ravel())
        want = cases.restated(c, got, z, dense, borders)
        for e, (g, (xy, kz)) in enumerate(zip(got, want)):
            assert dv.same_bits(g["xy"], xy) and dv.same_bits(g["z"], kz), (fmt, dense, e)
        kept = sum(len(w[1]) for w in want)
        with_outside = sum(len(w[1]) for w in cases.restated(c, got, np.where(inside, z, np.float32(1.0)), dense, borders))
        with_every_depth = sum(len(w[1]) for w in cases.restated(c, got, np.ones_like(z), dense, borders))
        print("undistort = 2, format %d, %s: %d keypoints; %d more with a depth at the raw positions outside the map, %d more with a depth everywhere" % (
            fmt, "every candidate" if dense else "grid", kept, with_outside - kept, with_every_depth - kept))
        assert kept == counts.sum() and with_outside - kept >= 1 and with_every_depth > with_outside
    finally:
        pb.close()


@pytest.mark.parametrize("dense", [False, True])
def test_launches_synchronisations_and_bytes(mbavo, gpu_ctx, dense):
    """Check 7: a prepare costs ceil((L-1)/3) + 4 launches (every_candidate: + 5), an update with keyframes what an undistort = 0
    object's costs, an update with n_key = 0 and a d_blur ceil((L-1)/3) + 1; one synchronisation each, 4 B L bytes back (none
    without keyframes).  Before set_camera prepare, update and track_frame return MBAVO_E_ARG and launch nothing; set_camera
    on an undistort = 0 object, or with a bad camera, returns MBAVO_E_ARG."""
    from mba_vo_amd import workloads
    capi = mbavo.capi
    c = cases.undistort_case("crop", "outside")
    B, keys = c["B"], [0, 2]
    kp = 3 if dense else 2
    raw = {k: dv.dev(v)[0] for k, v in c["raw"].items()}
    und = {k: dv.dev(v)[0] for k, v in c["und"].items()}
    z, new_z = dv.dev(c["z"], np.ascontiguousarray(c["new_z"][keys]))
    for L in (3, 1):
        pyr = (L - 1 + 2) // 3
        kw = dict(L=L, S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
        fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense, **kw), cases.undistort_batch(gpu_ctx, c, 0, dense, **kw)
        try:
            # no camera yet: nothing runs
            assert fused.stats()[:3] == (0, 0, 0)
            assert gpu_ctx.lib.mbavo_pairs_prepare(fused.handle, raw["sharp"].data_ptr(), z.data_ptr(), raw["blur"].data_ptr(), None) == E_ARG
            assert gpu_ctx.lib.mbavo_pairs_update(fused.handle, raw["blur"].data_ptr(), 0, None, None, None, None) == E_ARG
            frames = (capi.PairsFrame * B)()
            t = np.full(B, 0.1)
            assert gpu_ctx.lib.mbavo_pairs_track_frame(fused.handle, raw["blur"].data_ptr(), 0, None, None, None, capi.dp(t), capi.dp(t), C.byref(lms.lm_batch_opts(capi, 2, 3)),
                                                       None, None, 0, ps.FLOW0, ps.FLOW1, ps.KERNEL, frames, None) == E_ARG
            assert fused.stats()[:3] == (0, 0, 0) and fused.step_stats()[0] == (0, 0, 0) and fused.track_stats() == ((0, 0, 0), (0, 0, 0))
            assert twin.set_camera(cases.undistort_camera(c)) == E_ARG  # an undistort = 0 object has no camera
            for bad in (workloads.camera_radtan(0, c["Ws"], c["from_intr"], cases.DISTS["outside"]), workloads.camera_radtan(4096, 1025, c["from_intr"], cases.DISTS["outside"]),
                        workloads.camera_radtan(c["Hs"], c["Ws"], (0.0,) + tuple(c["from_intr"][1:]), cases.DISTS["outside"])):
                assert fused.set_camera(bad) == E_ARG
            assert gpu_ctx.lib.mbavo_pairs_set_camera(fused.handle, None) == E_ARG
            assert gpu_ctx.lib.mbavo_pairs_prepare(fused.handle, raw["sharp"].data_ptr(), z.data_ptr(), raw["blur"].data_ptr(), None) == E_ARG  # still none
            assert fused.set_camera(cases.undistort_camera(c)) == 0
            fused.prepare(raw["sharp"], z, raw["blur"])
            twin.prepare(und["sharp"], z, und["blur"])
            assert fused.stats()[:3] == (pyr + 2 + kp, 1, 4 * B * L), fused.stats()
            assert twin.stats()[:3] == (pyr + 1 + kp, 1, 4 * B * L)  # the remap is the one launch more: the copies were no kernels
            fused.update(raw["new_blur"], keys, raw["new_sharp"][keys].contiguous(), new_z)
            twin.update(und["new_blur"], keys, und["new_sharp"][keys].contiguous(), new_z)
            assert fused.step_stats()[0] == twin.step_stats()[0] == (1 + pyr + 1 + kp, 1, 4 * B * L)
            fused.update(None, keys, raw["new_sharp"][keys].contiguous(), new_z)
            twin.update(None, keys, und["new_sharp"][keys].contiguous(), new_z)
            assert fused.step_stats()[0] == twin.step_stats()[0]
            fused.update(raw["blur"])
            twin.update(und["blur"])
            assert fused.step_stats()[0] == (pyr + 1, 1, 0) and twin.step_stats()[0] == (pyr, 1, 0)
        finally:
            fused.close()
            twin.close()


@pytest.mark.parametrize("dense", [False, True])
def test_track_frame_on_raw_images_returns_the_same_frames(mbavo, gpu_ctx, dense):
    """Check 8: one mbavo_pairs_track_frame (new keyframes for pairs [0, 2], new blurred frames) on an undistort = 1 object and on
    an undistort = 0 object fed the remapped images: the same mbavo_pairs_frame bytes, LM results and trace records -- the
    arrays the LM reads are identical, so this is equality."""
    capi = mbavo.capi
    c = cases.undistort_case("crop", "outside")
    cases.witness(c)
    B, keys, k = c["B"], [0, 2], 2
    kw = dict(S=2, k=k, N=2, pattern=np.array([[0, 0]], np.int32))
    z, new_z = dv.dev(c["z"], np.ascontiguousarray(c["new_z"][keys]))
    runs = []
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense, **kw), cases.undistort_batch(gpu_ctx, c, 0, dense, **kw)
    try:
        assert fused.set_camera(cases.undistort_camera(c)) == 0
        for pb, src in ((fused, c["raw"]), (twin, c["und"])):
            pb.prepare(dv.dev(src["sharp"])[0], z, dv.dev(src["blur"])[0])
            runs.append(dv.frames_of(gpu_ctx, capi, pb, c, dv.dev(src["new_blur"])[0], keys, dv.dev(np.ascontiguousarray(src["new_sharp"][keys]))[0], new_z, k))
        (ff, cf, rf, tf), (ft, ct, rt, tt) = runs
        assert np.array_equal(cf, ct) and cf.min() > 0
        assert ff == ft and rf == rt and tf == tt and len(tf) > 0
        status = [capi.PairsFrame.from_buffer_copy(f).a.status for f in ff]
        assert status == [0] * B
    finally:
        fused.close()
        twin.close()
