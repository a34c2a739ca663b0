"""The unified camera on the device (mbavo_undistort_map_unified, mbavo_pairs_set_camera_unified) and the batched stand-alone
remap (mbavo_undistort_u8_batch).

The map is held bit for bit to the numpy restatement of include/mbavo.h's formulas (tests/pairs_unified_ref.py, whose model
tests/test_pairs_unified_api.py pins against the reference's own inverse).  Everything downstream of the map does not know the
camera model, so the batch is held the way tests/test_gpu_pairs_undistort.py holds the radial-tangential route, with its
helpers: an undistort = 1 object given raw unified images against an undistort = 0 object given the numpy-remapped images, every
array bit for bit after a prepare, an update (also across a change of the camera model on one object, both ways) and a
mbavo_pairs_track_frame; undistort = 2 against the restatement's look-up; launches, synchronisations and D2H bytes against the
radial-tangential route's.  The batched remap is held byte for byte to numpy and to n single calls, on image sizes that put the
second and third image off a word boundary.

Shapes: 48 x 64 from a 52 x 76 raw camera ("crop"), 50 x 70 from 50 x 70 ("same", an odd number of words), 45 x 63 (an odd number
of bytes); L = 3, B = 3.  Every test asserts the witness of the parameter set it relies on."""
import ctypes as C

import numpy as np
import pytest

import pairs_cases as cases
import pairs_device as dv
import pairs_undistort_ref as uref
import pairs_unified_ref as xref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
GEOMETRIES = {"crop": (48, 64, 52, 76), "same": (50, 70, 50, 70), "odd": (45, 63, 52, 76), "wide": (48, 64, 52, 76)}  # H, W, Hs, Ws

_CASES = {}


def _case(geometry, name):
    """Everything numpy of one (geometry, parameter set), made once and left unchanged: the map, raw images and depth maps of
    B = 3 pairs (and a second set for an update), their remapped versions.  The raw images are those of the radial-tangential
    tests (the same seeds), so that one object can be fed the same images under either camera."""
    key = (geometry, name)
    if key not in _CASES:
        H, W, Hs, Ws = GEOMETRIES[geometry]
        B, s = 3, xref.SETS[name]
        to_intr = xref.intrinsics(H, W)
        from_intr = xref.from_intrinsics(name, "crop" if geometry == "odd" else geometry, Hs, Ws)
        m = xref.undistort_map(from_intr, s["xi"], s["dist"], to_intr, H, W)
        tex = lambda seed: np.stack([synth.texture_image(Hs, Ws, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        raw = dict(sharp=tex(7), blur=tex(107), new_sharp=tex(40), new_blur=tex(140))
        und = {k: np.stack([uref.remap_u8(im, m) for im in v]) for k, v in raw.items()}
        rng = np.random.default_rng(5)
        z = rng.uniform(0.5, 3.0, (2, B, H, W)).astype(np.float32)  # depth in the undistorted geometry, with holes
        z[rng.uniform(0, 1, z.shape) < 0.15] = 0.0
        _CASES[key] = dict(shape=geometry, dist=name, H=H, W=W, Hs=Hs, Ws=Ws, L=3, B=B, intr=to_intr, from_intr=from_intr, xi=s["xi"],
                           coeffs=s["dist"], map=m, raw=raw, und=und, z=z[0], new_z=z[1], outside=uref.tap_outside(m, Hs, Ws))
    return _CASES[key]


def _camera(c):
    from mba_vo_amd import workloads
    return workloads.camera_unified(c["Hs"], c["Ws"], c["from_intr"], c["xi"], c["coeffs"])


@pytest.mark.parametrize("geometry", ["crop", "same"])
@pytest.mark.parametrize("name", ["outside", "inside", "pinhole"])
def test_map_equals_numpy_bit_for_bit(mbavo, gpu_ctx, geometry, name):
    """Check 1: every entry of the map, the last (odd) pixel pair included; also into a buffer that is only 8-byte aligned.  The
    xi = 0 set is the closed-form affine grid."""
    import torch
    from mba_vo_amd import workloads
    c = _case(geometry, name)
    cases.witness(c)
    H, W = c["H"], c["W"]
    got = workloads.undistort_map(gpu_ctx, _camera(c), c["intr"], H, W).cpu().numpy()
    assert got.dtype == np.float32 and dv.same_bits(got, c["map"])
    if name == "pinhole":
        assert dv.same_bits(got, xref.affine_grid(c["from_intr"], c["intr"], H, W))
    buf = torch.full((2 * H * W + 4,), -7.0, dtype=torch.float32, device="cuda:0")
    K = np.ascontiguousarray(c["intr"], np.float64)
    cam = _camera(c)
    assert gpu_ctx.lib.mbavo_undistort_map_unified(gpu_ctx.handle, C.byref(cam), mbavo.capi.dp(K), H, W, buf.data_ptr() + 8) == 0
    out = buf.cpu().numpy()
    assert dv.same_bits(out[2:-2].reshape(H, W, 2), c["map"]) and np.all(out[:2] == -7.0) and np.all(out[-2:] == -7.0)


def test_bad_arguments_are_rejected_without_a_launch(mbavo, gpu_ctx):
    """Check 2: MBAVO_E_ARG and poisoned output buffers left as they were: a NULL pointer, a size out of range, fx or fy equal to 0
    on either camera, a negative or non-finite xi; for the batched remap also n < 1 and n > 65535."""
    import torch
    from mba_vo_amd import workloads
    lib, capi, c = gpu_ctx.lib, mbavo.capi, _case("crop", "inside")
    H, W, Hs, Ws = c["H"], c["W"], c["Hs"], c["Ws"]
    K = np.ascontiguousarray(c["intr"], np.float64)
    out = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda:0")
    good = _camera(c)

    def cam(**kw):
        k = workloads.camera_unified(kw.get("H", Hs), kw.get("W", Ws), c["from_intr"], kw.get("xi", c["xi"]), c["coeffs"])
        for i in kw.get("zero", ()):
            k.intrinsics[i] = 0.0
        return k

    call = lambda k, to, h, w, o: lib.mbavo_undistort_map_unified(gpu_ctx.handle, C.byref(k) if k is not None else None,
                                                                  capi.dp(to) if to is not None else None, h, w, o)
    K0, K1 = K.copy(), K.copy()
    K0[0], K1[1] = 0.0, 0.0
    o = out.data_ptr()
    for args in ((None, K, H, W, o), (good, None, H, W, o), (good, K, H, W, None), (good, K, 0, W, o), (good, K, H, -1, o), (good, K, 2048, 2049, o),
                 (cam(H=0), K, H, W, o), (cam(W=0), K, H, W, o), (cam(H=4096, W=1025), K, H, W, o), (cam(zero=(0,)), K, H, W, o),
                 (cam(zero=(1,)), K, H, W, o), (good, K0, H, W, o), (good, K1, H, W, o), (cam(xi=-1e-300), K, H, W, o), (cam(xi=-1.0), K, H, W, o),
                 (cam(xi=float("nan")), K, H, W, o), (cam(xi=float("inf")), K, H, W, o), (cam(xi=float("-inf")), K, H, W, o)):
        assert call(*args) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    n = 2
    src = torch.zeros((n, Hs, Ws), dtype=torch.uint8, device="cuda:0")
    dst = torch.full((n, H, W), 0xA5, dtype=torch.uint8, device="cuda:0")
    s, m, d = src.data_ptr(), out.data_ptr(), dst.data_ptr()
    for args in ((None, n, Hs, Ws, m, H, W, d), (s, n, Hs, Ws, None, H, W, d), (s, n, Hs, Ws, m, H, W, None), (s, n, 0, Ws, m, H, W, d),
                 (s, n, Hs, Ws, m, H, 0, d), (s, n, 4096, 1025, m, H, W, d), (s, n, Hs, Ws, m, 2049, 2048, d), (s, 0, Hs, Ws, m, H, W, d),
                 (s, -1, Hs, Ws, m, H, W, d), (s, 65536, Hs, Ws, m, H, W, d), (s, -2147483648, Hs, Ws, m, H, W, d)):
        assert lib.mbavo_undistort_u8_batch(gpu_ctx.handle, *args) == E_ARG
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    assert call(cam(xi=0.0), K, H, W, o) == 0 and call(good, K, H, W, o) == 0  # xi = 0 is a camera; and good arguments write
    torch.cuda.synchronize()
    assert dv.same_bits(out.cpu().numpy(), c["map"])


@pytest.mark.parametrize("geometry", ["crop", "odd"])
@pytest.mark.parametrize("n", [1, 3])
def test_batched_remap_equals_numpy_and_single_calls(mbavo, gpu_ctx, geometry, n):
    """Check 3: 48 x 64 (whole words) and 45 x 63 (2835 bytes an image: images 1 and 2 start off a word boundary and the ragged
    end runs), through the distorting map with the entries the remap's rules are about planted in it; then with the destination
    and the map moved off their alignment.  Byte for byte numpy and n calls of mbavo_undistort_u8; guard bytes intact."""
    import torch
    from mba_vo_amd import workloads
    c = _case(geometry, "outside")
    assert 0.01 < cases.witness(c) < 0.10
    H, W, Hs, Ws = c["H"], c["W"], c["Hs"], c["Ws"]
    assert (H * W) % 4 == (0 if geometry == "crop" else 3)
    m = cases.special_map(c)
    want = np.stack([uref.remap_u8(im, m) for im in c["raw"]["sharp"][:n]])
    assert c["outside"].any() and (want == 0).any() and want.max() > 100  # the border rule and the planted entries are in play
    raw_t, map_t = dv.dev(np.ascontiguousarray(c["raw"]["sharp"][:n]), m)
    got = workloads.undistort_u8_batch(gpu_ctx, raw_t, map_t).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(workloads.undistort_u8(gpu_ctx, raw_t, map_t).cpu().numpy(), got)
    # guard bytes after the last image; then one to three bytes / one float off alignment
    for d_off, m_off in ((0, 0), (3, 1), (1, 0), (2, 1)):
        mbuf = torch.zeros(2 * H * W + 1, dtype=torch.float32, device="cuda:0")
        mbuf[m_off:m_off + 2 * H * W] = map_t.view(-1)
        dst = torch.full((n * H * W + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert gpu_ctx.lib.mbavo_undistort_u8_batch(gpu_ctx.handle, raw_t.data_ptr(), n, Hs, Ws, mbuf.data_ptr() + 4 * m_off, H, W, dst.data_ptr() + d_off) == 0
        out = dst.cpu().numpy()
        assert np.array_equal(out[d_off:d_off + n * H * W].reshape(n, H, W), want), (d_off, m_off)
        assert np.all(out[:d_off] == 0xA5) and np.all(out[d_off + n * H * W:] == 0xA5), (d_off, m_off)


@pytest.mark.parametrize("geometry,name", [("crop", "outside"), ("crop", "inside"), ("same", "outside")])
@pytest.mark.parametrize("kf", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_prepare_on_raw_images_equals_prepare_on_remapped_images(mbavo, gpu_ctx, geometry, name, kf, dense):
    """Check 4: B = 3, L = 3: every image level, gradient image (or packed word), keypoint, depth and count of the undistort = 1
    object after set_camera_unified equals the undistort = 0 object's on the numpy-remapped images."""
    c = _case(geometry, name)
    cases.witness(c)
    raw_s, raw_b, z, und_s, und_b = dv.dev(c["raw"]["sharp"], c["raw"]["blur"], c["z"], c["und"]["sharp"], c["und"]["blur"])
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense, kf), cases.undistort_batch(gpu_ctx, c, 0, dense, kf)
    try:
        assert fused.set_camera(_camera(c)) == 0
        cf, ct = fused.prepare(raw_s, z, raw_b), twin.prepare(und_s, z, und_b)
        assert np.array_equal(cf, ct) and cf.min() > 0
        got = dv.read_batch(fused, cf)
        dv.assert_twins(got, dv.read_batch(twin, ct), (geometry, name, kf, dense))
        for b in range(c["B"]):  # level 0 is the remapped image, the current frame too
            assert np.array_equal(got[b * c["L"]]["ref"], c["und"]["sharp"][b].ravel()) and np.array_equal(got[b * c["L"]]["cur"], c["und"]["blur"][b].ravel())
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("mode", ["keys and blur", "keys only", "blur only", "radtan to unified", "unified to radtan"])
@pytest.mark.parametrize("dense", [False, True])
def test_update_equals_a_fresh_prepare_of_the_composite_inputs(mbavo, gpu_ctx, mode, dense):
    """Check 5: key list [0, 2] of B = 3 with and without d_blur, n_key = 0 with a d_blur, and an update after the SAME object was
    given a camera of the other model (the images the update brings go through the new map, pair 1's keyframe keeps the old
    one) -- from a radial-tangential camera to a unified one and back.  The expectation is an undistort = 0 object prepared on the
    composite of the numpy-remapped images."""
    uni, rad = _case("crop", "outside"), cases.undistort_case("crop", "outside")
    cases.witness(uni), cases.witness(rad)
    for k in uni["raw"]:  # the same raw images under either camera: only the map differs
        assert np.array_equal(uni["raw"][k], rad["raw"][k])
    assert not np.array_equal(uni["und"]["new_sharp"], rad["und"]["new_sharp"]) and (uni["H"], uni["W"], uni["Hs"], uni["Ws"]) == (rad["H"], rad["W"], rad["Hs"], rad["Ws"])
    first, new = {"radtan to unified": (rad, uni), "unified to radtan": (uni, rad)}.get(mode, (uni, uni))
    camera = lambda c: cases.undistort_camera(c) if c is rad else _camera(c)
    c = uni
    B, keys = c["B"], ([] if mode == "blur only" else [0, 2])
    with_blur = mode != "keys only"
    sharp, depth = first["und"]["sharp"].copy(), c["z"].copy()
    sharp[keys], depth[keys] = new["und"]["new_sharp"][keys], c["new_z"][keys]
    blur = new["und"]["new_blur"] if with_blur else first["und"]["blur"]
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense), cases.undistort_batch(gpu_ctx, c, 0, dense)
    try:
        assert fused.set_camera(camera(first)) == 0
        before = fused.prepare(*dv.dev(c["raw"]["sharp"], c["z"], c["raw"]["blur"]))
        if new is not first:
            assert fused.set_camera(camera(new)) == 0
        args = [dv.dev(c["raw"]["new_blur"])[0] if with_blur else None, keys]
        if keys:
            args += dv.dev(np.ascontiguousarray(c["raw"]["new_sharp"][keys]), np.ascontiguousarray(c["new_z"][keys]))
        cf = fused.update(*args)
        ct = twin.prepare(*dv.dev(np.ascontiguousarray(sharp), np.ascontiguousarray(depth), np.ascontiguousarray(blur)))
        assert np.array_equal(cf, ct) and np.array_equal(cf[1], before[1]) and (not keys or not np.array_equal(cf[keys], before[keys]))
        got = dv.read_batch(fused, cf)
        dv.assert_twins(got, dv.read_batch(twin, ct), (mode, dense))
        assert np.array_equal(got[c["L"]]["ref"], first["und"]["sharp"][1].ravel())  # pair 1's keyframe: the first camera's
        if keys:
            assert np.array_equal(got[0]["ref"], new["und"]["new_sharp"][0].ravel())  # pair 0's: the camera of the last call
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_raw_geometry_depth_maps_are_looked_up_through_the_map(mbavo, gpu_ctx, fmt, dense):
    """Check 6: undistort = 2 with depth formats 0, 1 and 2, no border margin.  Kept keypoints and their z equal the restatement
    (the raw element nearest to the unified map's entry at the keypoint's level-0 pixel, format 1 with that pixel's ray).  The
    "wide" geometry points the two top and the two bottom rows of level 0 outside the raw map (the border rows themselves have no
    gradient, so one row each would show nothing); keypoints there are dropped: with a depth of 1 m at those pixels instead,
    the restatement keeps more."""
    c = _case("wide", "outside")
    B, o, borders = c["B"], cases.DEPTH_FORMATS[fmt], (0, 0, 0)
    raw_d = cases.raw_depth(fmt, B, c["Hs"], c["Ws"], seed=31 + fmt)
    inside = uref.nearest_raw(c["map"], c["Hs"], c["Ws"])[0]
    z = np.stack([uref.depth_through_map(fmt, raw_d[b], c["map"], c["intr"], o["depth_unit"], o["depth_max"]) for b in range(B)])
    assert (~inside).mean() > 0.03 and (~inside).all(1).sum() == 4 and np.all(z[:, ~inside] == 0)
    pb = cases.undistort_batch(gpu_ctx, c, 2, dense, depth=fmt, borders=borders)
    try:
        assert pb.set_camera(_camera(c)) == 0
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
        assert kept == counts.sum() and with_outside - kept >= 1
    finally:
        pb.close()


@pytest.mark.parametrize("dense", [False, True])
def test_launches_synchronisations_and_bytes_are_those_of_the_radtan_route(mbavo, gpu_ctx, dense):
    """Check 7: an object given a unified camera and one given a radial-tangential camera report the same launches,
    synchronisations and D2H bytes after a prepare and after each kind of update, and those are the documented ones: a prepare
    ceil((L-1)/3) + 4 launches (every_candidate: + 5), an update with n_key = 0 and a d_blur ceil((L-1)/3) + 1.
    set_camera_unified itself waits for nothing, needs undistort != 0 and rejects a bad camera, leaving the object without one."""
    uni, rad = _case("crop", "outside"), cases.undistort_case("crop", "outside")
    c, B, keys = uni, uni["B"], [0, 2]
    kp = 3 if dense else 2
    raw = {k: dv.dev(v)[0] for k, v in c["raw"].items()}
    z, new_z = dv.dev(c["z"], np.ascontiguousarray(c["new_z"][keys]))
    from mba_vo_amd import workloads
    for L in (3, 1):
        pyr = (L - 1 + 2) // 3
        kw = dict(L=L, S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
        a, b, plain = cases.undistort_batch(gpu_ctx, c, 1, dense, **kw), cases.undistort_batch(gpu_ctx, c, 1, dense, **kw), cases.undistort_batch(gpu_ctx, c, 0, dense, **kw)
        try:
            assert plain.set_camera(_camera(c)) == E_ARG  # an undistort = 0 object has no camera
            for bad in (workloads.camera_unified(0, c["Ws"], c["from_intr"], 1.0), workloads.camera_unified(c["Hs"], c["Ws"], c["from_intr"], -0.5),
                        workloads.camera_unified(c["Hs"], c["Ws"], c["from_intr"], float("nan")),
                        workloads.camera_unified(c["Hs"], c["Ws"], (0.0,) + tuple(c["from_intr"][1:]), 1.0)):
                assert a.set_camera(bad) == E_ARG
            assert gpu_ctx.lib.mbavo_pairs_set_camera_unified(a.handle, None) == E_ARG
            assert gpu_ctx.lib.mbavo_pairs_prepare(a.handle, raw["sharp"].data_ptr(), z.data_ptr(), raw["blur"].data_ptr(), None) == E_ARG  # still no camera
            assert a.stats()[:3] == (0, 0, 0)
            assert a.set_camera(_camera(uni)) == 0 and b.set_camera(cases.undistort_camera(rad)) == 0
            assert a.stats()[:3] == (0, 0, 0)  # (the map's launch belongs to no prepare; nothing was waited for)
            for pb in (a, b):
                pb.prepare(raw["sharp"], z, raw["blur"])
            assert a.stats()[:3] == b.stats()[:3] == (pyr + 2 + kp, 1, 4 * B * L), (a.stats(), b.stats())
            assert a.stats()[3] == b.stats()[3]  # one map either way
            for pb in (a, b):
                pb.update(raw["new_blur"], keys, raw["new_sharp"][keys].contiguous(), new_z)
            assert a.step_stats()[0] == b.step_stats()[0] == (1 + pyr + 1 + kp, 1, 4 * B * L)
            for pb in (a, b):
                pb.update(None, keys, raw["new_sharp"][keys].contiguous(), new_z)
            assert a.step_stats()[0] == b.step_stats()[0]
            for pb in (a, b):
                pb.update(raw["blur"])
            assert a.step_stats()[0] == b.step_stats()[0] == (pyr + 1, 1, 0)
        finally:
            a.close()
            b.close()
            plain.close()


@pytest.mark.parametrize("dense", [False, True])
def test_track_frame_on_raw_images_returns_the_same_frames(mbavo, gpu_ctx, dense):
    """Check 8: one mbavo_pairs_track_frame (new keyframes for pairs [0, 2], new blurred frames) on an undistort = 1 object with a
    unified camera and on an undistort = 0 object fed the numpy-remapped images: the same mbavo_pairs_frame bytes, LM results and
    trace records -- the arrays the LM reads are identical, so this is equality."""
    capi = mbavo.capi
    c = _case("crop", "outside")
    cases.witness(c)
    B, keys, k = c["B"], [0, 2], 2
    kw = dict(S=2, k=k, N=2, pattern=np.array([[0, 0]], np.int32))
    z, new_z = dv.dev(c["z"], np.ascontiguousarray(c["new_z"][keys]))
    runs = []
    fused, twin = cases.undistort_batch(gpu_ctx, c, 1, dense, **kw), cases.undistort_batch(gpu_ctx, c, 0, dense, **kw)
    try:
        assert fused.set_camera(_camera(c)) == 0
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
