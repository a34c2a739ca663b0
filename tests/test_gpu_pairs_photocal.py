"""The photometric calibration at intake on the device (mbavo_pairs_set_photometric, _clear_photometric, _photocal_stats,
mbavo_photometric_u8_batch) against the numpy restatement (tests/pairs_photocal_ref.py), bit for bit.

Objects: B = 3, L = 1, 9 x 17 (153 pixels: an odd count, a ragged last lane, images 1 and 2 of a packed array off a word, and with
G = 2 the second camera's map and vignette off the 16-byte boundary), raw size 11 x 19.  Every configuration: undistort 0 and 1,
radial-tangential and unified cameras, one camera and G = 2 with the pairs assigned 0, 1, 0.  The calibration: a gamma table per
camera and a random vignette in [0.03, 1] -- it crosses v_min = 0.0625 and saturates taps at 255 -- with one NaN and one 0.
The hand-off to the pyramid, gradients and keypoints is held on a second object, L = 3 at 32 x 40.

Sizes and alignments the kernels branch on (the tests below test_plain_load_variants_in_a_child_process): a workgroup of
k_pairs_photocal_level0 and k_photometric_u8_batch takes 4096 pixels, one of the calibrated remap 1024, one of
k_photocal_inverse_vignette 1024 floats.  G = 2 pinhole objects at 64 x 80 (5120 pixels: two workgroups per image, every lane of
both cameras on the 16-byte path) and 65 x 67 (4355, odd: the second workgroup holds a ragged end, camera 1's vignette is off 16
bytes); a raw G = 2 object with 72 x 100 from 80 x 112 (eight workgroups per row; a prepare takes the `both` kernel, an update with a
key list the per-row kernel); the stand-alone call at both sizes, also on pointers one byte into an allocation; and the inverse
vignette kernel, seen through the bytes of an identity table, on a caller's pointer off 16 bytes, under three v_min and on every
special value a float can hold."""
import ctypes as C

import numpy as np
import pytest

import pairs_cameras_ref as cref
import pairs_device as dv
import pairs_oracle as po
import pairs_photocal_ref as pc
import pairs_undistort_ref as uref
import pairs_unified_ref as xref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
B, H, W, HS, WS = 3, 9, 17, 11, 19
IDX = (0, 1, 0)
CONFIGS = [(u, model, G) for u in (0, 1) for model in (1, 2) for G in (0, 2)]
_CASES = {}


def _cams(model, h=H, w=W, hs=HS, ws=WS):
    """Two cameras of one model whose undistorted images are h x w; the second is off the first in every entry."""
    K = uref.intrinsics(h, w)
    K2 = (1.03 * K[0], 0.98 * K[1], K[2] + 0.4, K[3] - 0.3)
    if model == 2:
        s = xref.SETS["inside"]
        f = xref.from_intrinsics("inside", "crop", hs, ws)
        return [dict(model=2, Hs=hs, Ws=ws, from_intr=f, xi=s["xi"], dist=s["dist"], to_intr=K),
                dict(model=2, Hs=hs, Ws=ws, from_intr=f, xi=0.9 * s["xi"], dist=s["dist"], to_intr=K2)]
    f = uref.intrinsics(hs, ws)
    return [dict(model=1, Hs=hs, Ws=ws, from_intr=f, xi=0.0, dist=uref.DIST_OUTSIDE, to_intr=K),
            dict(model=1, Hs=hs, Ws=ws, from_intr=f, xi=0.0, dist=uref.DIST_INSIDE, to_intr=K2)]


def _case(h=H, w=W, hs=HS, ws=WS):
    """Everything numpy of one size, made once and left unchanged: images in both geometries, depth maps, tables, vignettes."""
    key = (h, w)
    if key not in _CASES:
        rng = np.random.default_rng(43 + h)
        tex = lambda hh, ww, seed: np.stack([synth.texture_image(hh, ww, seed=seed + 3 * b, octaves=(8, 4, 2)) for b in range(B)])
        seeds = dict(sharp=7, blur=107, new_sharp=40, new_blur=140, blur3=171)
        G = np.stack([pc.gamma_G(2.2), pc.gamma_G(1.8)])
        luts = np.stack([pc.table(G[0], 0.5), pc.table(G[1], 0.7)])
        vig = {}
        for name, (hh, ww) in dict(pin=(h, w), raw=(hs, ws)).items():
            V = rng.uniform(0.03, 1.0, (2, hh, ww)).astype(np.float32)
            V[0, 1, 2], V[0, 2, 5], V[1, 3, 3], V[1, 4, 1] = np.nan, 0.0, 0.0, np.nan
            vig[name] = V
        _CASES[key] = dict(pin={k: tex(h, w, s) for k, s in seeds.items()}, raw={k: tex(hs, ws, s) for k, s in seeds.items()},
                           depth=rng.uniform(1.0, 3.0, (B, h, w)).astype(np.float32), G=G, luts=luts, V=vig,
                           inv={k: pc.inverse_vignette(v) for k, v in vig.items()}, H=h, W=w, Hs=hs, Ws=ws)
    return _CASES[key]


def _object(ctx, c, undistort, model, G, L=1, cams=None):
    """(object, the maps of its cameras or None, the calibration of every pair).  cams: two cameras in place of _cams(model)'s."""
    from mba_vo_amd import workloads
    cams = _cams(model, c["H"], c["W"], c["Hs"], c["Ws"]) if cams is None else cams
    pb = workloads.PairBatch(ctx, B, L=L, H=c["H"], W=c["W"], S=3, k=2, N=2, intr=cams[0]["to_intr"], border=2, cell=3, thresh=1.0,
                             undistort=undistort, num_cameras=G)
    single = lambda cam: (workloads.camera_unified(cam["Hs"], cam["Ws"], cam["from_intr"], cam["xi"], cam["dist"]) if cam["model"] == 2
                          else workloads.camera_radtan(cam["Hs"], cam["Ws"], cam["from_intr"], cam["dist"]))
    if G:
        assert pb.set_cameras([workloads.pairs_camera(single(cam), cam["to_intr"]) for cam in cams], IDX) == 0
    elif undistort:
        assert pb.set_camera(single(cams[0])) == 0
    maps = cref.maps_of(cams, c["H"], c["W"]) if undistort else None
    return pb, maps, (IDX if G else (0, 0, 0))


def _n(G):
    return max(1, G)


def _expected(c, undistort, maps, cal, which, rows=range(B), vignette=True, luts=None):
    """Level 0 of the images `which` of the listed pairs as the restatement takes them in."""
    luts = c["luts"] if luts is None else luts
    geo = "raw" if undistort else "pin"
    out = []
    for b in rows:
        g = cal[b]
        inv = c["inv"][geo][g] if vignette else None
        img = c[geo][which][b]
        out.append(pc.remap(img, maps[g], luts[g], inv) if undistort else pc.pinhole(img, luts[g], inv))
    return out


def _images(c, undistort, which, rows=None):
    a = c["raw" if undistort else "pin"][which]
    return dv.dev(np.ascontiguousarray(a if rows is None else a[list(rows)]))[0]


def _level0(pb, counts):
    got = dv.read_batch(pb, counts)
    return [got[b * pb.L]["ref"] for b in range(B)], [got[b * pb.L]["cur"] for b in range(B)], got


def _same(got, want, tag):
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w.ravel()), (tag, b, int((g != w.ravel()).sum()))


@pytest.mark.parametrize("undistort,model,G", CONFIGS)
def test_every_intake_path_bit_for_bit_and_counted(mbavo, gpu_ctx, undistort, model, G):
    """prepare, update with a key list, update without one, track_frame and prepare_points under the calibration give the
    restatement's level-0 bytes, pairs that are not listed keep theirs; the identity calibration and clear_photometric give the bytes
    and the stats of the object before set_photometric; launches, synchronisations and D2H bytes are what the header states."""
    c = _case()
    n = _n(G)
    pb, maps, cal = _object(gpu_ctx, c, undistort, model, G)
    depth = dv.dev_depth(c["depth"])
    extra = 1 if undistort == 0 else 0  # one launch where the strided copies were
    try:
        assert pb.photocal_stats() == (0, 0, 0)
        # the object as it is today
        counts0 = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        plain, stats0 = dv.read_batch(pb, counts0), pb.stats()
        assert counts0.sum() > 0
        pb.update(_images(c, undistort, "new_blur"), [1], _images(c, undistort, "new_sharp", [1]), dv.dev_depth(c["depth"][[1]]))
        upd0 = pb.step_stats()[0]
        pb.update(_images(c, undistort, "blur3"))
        upd0_nokey = pb.step_stats()[0]
        # rejected calls change nothing
        o_bad = [dict(scale=1.5), dict(scale=-1.0), dict(v_min=-0.1), dict(v_min=float("nan")), dict(v_min=float("inf"))]
        for kw in o_bad:
            assert pb.set_photometric(c["G"][:n], None, **kw) == E_ARG
        bad_G = c["G"][:n].copy()
        bad_G[n - 1, 9] = bad_G[n - 1, 8] - 1.0
        assert pb.set_photometric(bad_G) == E_ARG
        assert gpu_ctx.lib.mbavo_pairs_set_photometric(pb.handle, n + 1, None, None, None) == E_ARG
        assert pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur")).tolist() == counts0.tolist()
        assert pb.stats() == stats0 and pb.photocal_stats() == (0, 0, 0)
        # the identity calibration: today's bytes, one launch more where the copies were
        assert pb.set_photometric() == 0 and pb.photocal_stats() == (0, 0, 0)
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        dv.assert_twins(dv.read_batch(pb, counts), plain, "identity")
        assert pb.stats() == (stats0[0] + extra,) + stats0[1:]
        ones = dv.dev(np.ones_like(c["V"]["raw" if undistort else "pin"][:n]))[0]
        assert pb.set_photometric(None, ones) == 0 and pb.photocal_stats() == (1, 0, 0)
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        dv.assert_twins(dv.read_batch(pb, counts), plain, "identity with a vignette of ones")
        # the calibration: gamma tables and the random vignette
        V = dv.dev(np.ascontiguousarray(c["V"]["raw" if undistort else "pin"][:n]))[0]
        scales = (0.5, 0.7)
        if n == 2:  # (one scale per call: camera 1's table is made under camera 0's scale here)
            luts = np.stack([pc.table(c["G"][0], 0.5), pc.table(c["G"][1], 0.5)])
        else:
            luts = c["luts"]
        assert pb.set_photometric(c["G"][:n], V, scale=scales[0]) == 0 and pb.photocal_stats() == (1, 0, 0)
        # a rejected call changes nothing, the statistics of the call before included
        assert pb.set_photometric(c["G"][:n], V, scale=2.0) == E_ARG and pb.set_photometric(bad_G, V) == E_ARG and pb.photocal_stats() == (1, 0, 0)
        if undistort:  # the object holds vignettes of the raw size: a camera call that brings another one is rejected
            from mba_vo_amd import workloads
            cams = _cams(model, H, W, HS + 1, WS)
            if G:
                other = [workloads.pairs_camera(workloads.camera_radtan(HS + 1, WS, cam["from_intr"], uref.DIST_NONE), cam["to_intr"]) for cam in cams]
                assert pb.set_cameras(other, IDX) == E_ARG
            else:
                assert pb.set_camera(workloads.camera_radtan(HS + 1, WS, cams[0]["from_intr"], uref.DIST_NONE)) == E_ARG
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        ref0, cur0, _ = _level0(pb, counts)
        want_ref, want_cur = _expected(c, undistort, maps, cal, "sharp", luts=luts), _expected(c, undistort, maps, cal, "blur", luts=luts)
        _same(ref0, want_ref, "prepare keyframes")
        _same(cur0, want_cur, "prepare current frames")
        assert pb.stats() == (stats0[0] + extra,) + stats0[1:]
        # (the inputs reach every branch: dead vignette pixels, saturated bytes, bytes that differ from the uncalibrated path)
        inv = c["inv"]["raw" if undistort else "pin"][:n]
        assert (inv == 0).any() and (np.concatenate([w.ravel() for w in want_ref]) == 255).any()
        assert any(not np.array_equal(w.ravel(), p["ref"]) for w, p in zip(want_ref, plain))
        # update: a key list of one pair, a new current frame for all; the others keep their keyframes
        counts = pb.update(_images(c, undistort, "new_blur"), [1], _images(c, undistort, "new_sharp", [1]), dv.dev_depth(c["depth"][[1]]))
        ref1, cur1, _ = _level0(pb, counts)
        new_ref = _expected(c, undistort, maps, cal, "new_sharp", rows=[1], luts=luts)[0]
        _same(ref1, [want_ref[0], new_ref, want_ref[2]], "update keyframes")
        _same(cur1, _expected(c, undistort, maps, cal, "new_blur", luts=luts), "update current frames")
        assert pb.step_stats()[0] == upd0  # (one launch where the scatter was)
        counts = pb.update(_images(c, undistort, "blur3"))
        ref2, cur2, _ = _level0(pb, counts)
        _same(ref2, [want_ref[0], new_ref, want_ref[2]], "update without keys: keyframes stay")
        _same(cur2, _expected(c, undistort, maps, cal, "blur3", luts=luts), "update without keys")
        assert pb.step_stats()[0] == (upd0_nokey[0] + extra,) + upd0_nokey[1:]
        # track_frame once (3 LM iterations): its intake is the update's
        _, counts_t, _, _ = dv.frames_of(gpu_ctx, mbavo.capi, pb, dict(B=B), _images(c, undistort, "blur"), (), None, None, 2)
        _same(_level0(pb, counts_t)[1], want_cur, "track_frame")
        # prepare_points once
        pts = [(np.array([[4.0, 4.0], [9.0, 5.0], [12.0, 3.0]]), np.array([1.5, 2.0, 2.5]))] * B
        counts_p = pb.prepare_points(_images(c, undistort, "new_sharp"), _images(c, undistort, "new_blur"), pts)
        ref3, cur3, _ = _level0(pb, counts_p)
        _same(ref3, _expected(c, undistort, maps, cal, "new_sharp", luts=luts), "prepare_points keyframes")
        _same(cur3, _expected(c, undistort, maps, cal, "new_blur", luts=luts), "prepare_points current frames")
        # a table without a vignette: no map is read
        assert pb.set_photometric(c["G"][:n], None, scale=0.5) == 0 and pb.photocal_stats() == (0, 0, 0)
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        _same(_level0(pb, counts)[0], _expected(c, undistort, maps, cal, "sharp", vignette=False, luts=luts), "no vignette")
        # and back
        assert pb.clear_photometric() == 0
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        dv.assert_twins(dv.read_batch(pb, counts), plain, "cleared")
        assert pb.stats() == stats0
        pb.update(_images(c, undistort, "blur3"))
        assert pb.step_stats()[0] == upd0_nokey
    finally:
        pb.close()


def test_set_photometric_needs_the_camera_first(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    c = _case()
    pb = workloads.PairBatch(gpu_ctx, B, L=1, H=H, W=W, S=3, k=2, N=2, border=2, cell=3, thresh=1.0, undistort=1)
    try:
        assert pb.set_photometric() == E_ARG and pb.photocal_stats() == (0, 0, 0)
    finally:
        pb.close()


@pytest.mark.parametrize("undistort", [0, 1])
def test_hand_off_to_pyramid_gradients_and_keypoints(mbavo, gpu_ctx, undistort):
    """L = 3 at 32 x 40 (raw 36 x 46): every level, the gradients, the keypoints and their counts equal those of a plain pinhole
    object that is handed the restatement's corrected level-0 images."""
    from mba_vo_amd import workloads
    c = _case(32, 40, 36, 46)
    pb, maps, cal = _object(gpu_ctx, c, undistort, 1, 0, L=3)
    plain = workloads.PairBatch(gpu_ctx, B, L=3, H=32, W=40, S=3, k=2, N=2, intr=_cams(1, 32, 40, 36, 46)[0]["to_intr"], border=2, cell=3, thresh=1.0)
    try:
        V = dv.dev(np.ascontiguousarray(c["V"]["raw" if undistort else "pin"][:1]))[0]
        assert pb.set_photometric(c["G"][:1], V, scale=0.5) == 0
        depth = dv.dev_depth(c["depth"])
        counts = pb.prepare(_images(c, undistort, "sharp"), depth, _images(c, undistort, "blur"))
        sharp = np.stack(_expected(c, undistort, maps, cal, "sharp"))
        blur = np.stack(_expected(c, undistort, maps, cal, "blur"))
        want = plain.prepare(dv.dev(sharp)[0], depth, dv.dev(blur)[0])
        assert counts.tolist() == want.tolist() and counts.sum() > 0
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(plain, want), ("hand-off", undistort))
    finally:
        pb.close()
        plain.close()


@pytest.mark.parametrize("vignette", [True, False])
def test_stand_alone_batch_equals_the_restatement(mbavo, gpu_ctx, vignette):
    """n_img = 5, n_cal = 2 with an index list, out of place and in place; 9 x 17 images (four of five start off a word) and 16 x 32
    (every lane on the 16-byte path)."""
    import torch
    from mba_vo_amd import workloads
    rng = np.random.default_rng(9)
    idx = [0, 1, 1, 0, 1]
    luts = _case()["luts"]
    for h, w in ((9, 17), (16, 32)):
        src = rng.integers(0, 256, (5, h, w), dtype=np.uint8)
        V = rng.uniform(0.03, 1.0, (2, h, w)).astype(np.float32)
        V[0, 0, 0], V[1, 1, 1] = np.nan, 0.0
        inv = pc.inverse_vignette(V)
        want = np.stack([pc.pinhole(src[i], luts[g], inv[g] if vignette else None) for i, g in enumerate(idx)])
        d_src, d_inv = dv.dev(src)[0], (dv.dev(inv)[0] if vignette else None)
        out = workloads.photometric_u8_batch(gpu_ctx, d_src, luts, d_inv, idx)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(d_src.cpu().numpy(), src), (h, w)
        workloads.photometric_u8_batch(gpu_ctx, d_src, luts, d_inv, idx, out=d_src)
        torch.cuda.synchronize()
        assert np.array_equal(d_src.cpu().numpy(), want), (h, w, "in place")
        # without a list: one calibration for all
        one = workloads.photometric_u8_batch(gpu_ctx, dv.dev(src)[0], luts[1:], d_inv[1:].contiguous() if vignette else None)
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), np.stack([pc.pinhole(s, luts[1], inv[1] if vignette else None) for s in src]))
    # an index outside the calibrations; no list with n_cal neither 1 nor n_img: rejected, nothing launched
    lib, fp = gpu_ctx.lib, np.ascontiguousarray(luts).ctypes.data_as(C.POINTER(C.c_float))
    bad = np.array([0, 2, 0, 0, 0], np.int32)
    assert lib.mbavo_photometric_u8_batch(gpu_ctx.handle, 5, d_src.data_ptr(), 16, 32, 2, fp, None, mbavo.capi.ip(bad), d_src.data_ptr()) == E_ARG
    assert lib.mbavo_photometric_u8_batch(gpu_ctx.handle, 5, d_src.data_ptr(), 16, 32, 2, fp, None, None, d_src.data_ptr()) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), want)


def test_plain_load_variants_in_a_child_process(mbavo, gpu_ctx):
    """MBAVO_PAIRS_PHOTOCAL_LDS=0 selects the kernels that read the table by plain loads (the A/B of tools/pairs_photocal_bench.py).
    The environment is read once per process, so a fresh child runs one pinhole configuration, one raw configuration with a
    camera set and the stand-alone call under the switch: the same bit-for-bit checks."""
    import os
    import subprocess
    import sys
    assert gpu_ctx.lib.mbavo_pairs_photocal_opts_size() == 32
    env = dict(os.environ, MBAVO_PAIRS_PHOTOCAL_LDS="0")
    pick = "(test_every_intake_path and (0-1-0 or 1-1-2)) or test_stand_alone_batch"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", pick],
                       env=env, capture_output=True, text=True, timeout=120, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "4 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- sizes and alignments the kernels branch on
def _prepare_and_update(ctx, c, undistort, pb, maps, cal, luts, tag):
    """A prepare, then an update with the key list [1], under (gamma tables, random vignettes) at scale 0.5: level 0 against the
    restatement; the pairs that are not listed keep their keyframes."""
    n = 2
    V = dv.dev(np.ascontiguousarray(c["V"]["raw" if undistort else "pin"][:n]))[0]
    assert pb.set_photometric(c["G"][:n], V, scale=0.5) == 0 and pb.photocal_stats() == (1, 0, 0)
    counts = pb.prepare(_images(c, undistort, "sharp"), dv.dev_depth(c["depth"]), _images(c, undistort, "blur"))
    ref0, cur0, _ = _level0(pb, counts)
    want_ref = _expected(c, undistort, maps, cal, "sharp", luts=luts)
    _same(ref0, want_ref, (tag, "prepare keyframes"))
    _same(cur0, _expected(c, undistort, maps, cal, "blur", luts=luts), (tag, "prepare current frames"))
    both = np.concatenate([w.ravel() for w in want_ref])
    assert (both == 255).any() and (both == 0).any()
    counts = pb.update(_images(c, undistort, "new_blur"), [1], _images(c, undistort, "new_sharp", [1]), dv.dev_depth(c["depth"][[1]]))
    ref1, cur1, _ = _level0(pb, counts)
    new_ref = _expected(c, undistort, maps, cal, "new_sharp", rows=[1], luts=luts)[0]
    assert not np.array_equal(new_ref, want_ref[1])
    _same(ref1, [want_ref[0], new_ref, want_ref[2]], (tag, "update keyframes"))
    _same(cur1, _expected(c, undistort, maps, cal, "new_blur", luts=luts), (tag, "update current frames"))


@pytest.mark.parametrize("h,w", [(64, 80), (65, 67)])
def test_pinhole_camera_set_over_two_workgroups(mbavo, gpu_ctx, h, w):
    c = _case(h, w, h + 4, w + 6)
    assert 4096 < h * w <= 8192 and ((h * w) % 4 == 0) == (h == 64)
    pb, maps, cal = _object(gpu_ctx, c, 0, 1, 2)
    try:
        luts = np.stack([pc.table(c["G"][0], 0.5), pc.table(c["G"][1], 0.5)])
        _prepare_and_update(gpu_ctx, c, 0, pb, maps, cal, luts, (h, w))
    finally:
        pb.close()


def test_raw_camera_set_over_eight_workgroups(mbavo, gpu_ctx):
    """72 x 100 from 80 x 112 raw images of object C's camera and a second one with another xi."""
    cam = po._C_CAM
    t = cam["to_intr"]
    cams = [cam, dict(cam, xi=0.7, to_intr=(1.02 * t[0], 0.99 * t[1], t[2] + 0.3, t[3] - 0.2))]
    c = _case(72, 100, cam["Hs"], cam["Ws"])
    assert (c["Hs"], c["Ws"]) == (80, 112) and (72 * 100 + 1023) // 1024 == 8
    pb, maps, cal = _object(gpu_ctx, c, 1, 2, 2, cams=cams)
    try:
        assert not np.array_equal(maps[0], maps[1])
        luts = np.stack([pc.table(c["G"][0], 0.5), pc.table(c["G"][1], 0.5)])
        _prepare_and_update(gpu_ctx, c, 1, pb, maps, cal, luts, "raw 72 x 100")
    finally:
        pb.close()


@pytest.mark.parametrize("vignette", [True, False])
def test_batch_call_over_two_workgroups_and_off_a_word(mbavo, gpu_ctx, vignette):
    """mbavo_photometric_u8_batch at 65 x 67 and 64 x 80: five images, two calibrations, out of place and in place; once more with
    d_src and d_dst one byte into a larger allocation, where every lane takes the byte loop across two workgroups."""
    import torch
    from mba_vo_amd import workloads
    rng = np.random.default_rng(11)
    idx = [0, 1, 1, 0, 1]
    luts = _case()["luts"]
    for h, w in ((65, 67), (64, 80)):
        n = 5 * h * w
        src = rng.integers(0, 256, (5, h, w), dtype=np.uint8)
        V = rng.uniform(0.03, 1.0, (2, h, w)).astype(np.float32)
        V[0, 0, 0], V[1, 1, 1], V[1, h - 1, w - 1] = np.nan, 0.0, 0.05
        inv = pc.inverse_vignette(V)
        want = np.stack([pc.pinhole(src[i], luts[g], inv[g] if vignette else None) for i, g in enumerate(idx)])
        assert (want == 255).any() == vignette and not np.array_equal(want, src)
        d_inv = dv.dev(inv)[0] if vignette else None
        for off in (0, 1):
            big_src = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda:0")
            big_dst = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda:0")
            d_src, d_dst = big_src[off:off + n].view(5, h, w), big_dst[off:off + n].view(5, h, w)
            d_src.copy_(torch.from_numpy(src))
            assert d_src.data_ptr() % 4 == off and d_dst.data_ptr() % 16 == off
            workloads.photometric_u8_batch(gpu_ctx, d_src, luts, d_inv, idx, out=d_dst)
            torch.cuda.synchronize()
            assert np.array_equal(d_dst.cpu().numpy(), want) and np.array_equal(d_src.cpu().numpy(), src), (h, w, off)
            workloads.photometric_u8_batch(gpu_ctx, d_src, luts, d_inv, idx, out=d_src)
            torch.cuda.synchronize()
            assert np.array_equal(d_src.cpu().numpy(), want), (h, w, off, "in place")
            for big, fill in ((big_src, 7), (big_dst, 9)):  # nothing outside the images was written
                edge = big.cpu().numpy()
                assert (edge[:off] == fill).all() and (edge[off + n:] == fill).all(), (h, w, off)


_SPECIALS = [np.nan, np.inf, -np.inf, -0.0, -0.5, 1e-39, float(np.finfo(np.float32).max), 0.0625, float(np.nextafter(np.float32(0.0625), np.float32(0))),
             1.5, 3.0, 0.0, float(np.finfo(np.float32).tiny)]


@pytest.mark.parametrize("v_min", [0.0, 0.2, 1e-40])
def test_inverse_vignette_kernel_through_the_bytes(mbavo, gpu_ctx, v_min):
    """The table is the identity, so a byte is u8(raw * inv) (pinhole) or the blend of such taps (raw).  A one-camera pinhole object
    at 9 x 17 takes its vignette, 153 floats, as a view one float into a larger tensor: every lane of k_photocal_inverse_vignette goes
    float by float and the last one is ragged.  A raw G = 2 object takes 2 x 36 x 46 floats: four workgroups on the 16-byte path.  Both
    vignettes hold _SPECIALS.  With v_min = 1e-40 the subnormal passes, its inverse is inf, and code 0 under it saturates (0 * inf)."""
    import torch
    rng = np.random.default_rng(21)
    identity = pc.table()
    assert np.array_equal(identity, np.arange(256, dtype=np.float32))

    def vignettes(n, hh, ww):
        V = rng.uniform(0.05, 1.6, (n, hh, ww)).astype(np.float32)
        for g in range(n):
            at = rng.permutation(hh * ww)[:2 * len(_SPECIALS)]
            V[g].ravel()[at] = np.array(_SPECIALS + _SPECIALS, np.float32)
        return V

    # pinhole, one camera, the caller's pointer off 16 bytes
    c = _case()
    V = vignettes(1, H, W)
    raw = np.ascontiguousarray(c["pin"]["sharp"]).copy()
    sub = np.argwhere(V[0] == np.float32(1e-39))
    raw[:, sub[0][0], sub[0][1]], raw[:, sub[1][0], sub[1][1]] = 0, 200  # code 0 and a bright code under the subnormal
    inv = pc.inverse_vignette(V, v_min)
    assert np.isinf(inv).any() == (v_min == 1e-40) and (inv == 0).any() and (inv == 16.0).any() == (v_min != 0.2)
    pb, _, _ = _object(gpu_ctx, c, 0, 1, 0)
    try:
        big = torch.zeros(H * W + 8, dtype=torch.float32, device="cuda:0")
        view = big[1:1 + H * W]
        view.copy_(torch.from_numpy(V.ravel()))
        assert view.data_ptr() % 16 == 4 and (H * W) % 4 == 1
        assert pb.set_photometric(None, view, v_min=v_min) == 0 and pb.photocal_stats() == (1, 0, 0)
        counts = pb.prepare(dv.dev(raw)[0], dv.dev_depth(c["depth"]), _images(c, 0, "blur"))
        ref0, cur0, _ = _level0(pb, counts)
        want = [pc.pinhole(raw[b], identity, inv[0]) for b in range(B)]
        _same(ref0, want, ("pinhole", v_min))
        _same(cur0, [pc.pinhole(c["pin"]["blur"][b], identity, inv[0]) for b in range(B)], ("pinhole current", v_min))
        if v_min == 1e-40:
            assert all(w[sub[0][0], sub[0][1]] == 255 and w[sub[1][0], sub[1][1]] == 255 for w in want)
        else:
            assert all(w[sub[0][0], sub[0][1]] == 0 and w[sub[1][0], sub[1][1]] == 0 for w in want)
    finally:
        pb.close()
    # raw, two cameras, two workgroups and more on the vector path
    c = _case(32, 40, 36, 46)
    V = vignettes(2, 36, 46)
    inv = pc.inverse_vignette(V, v_min)
    pb, maps, cal = _object(gpu_ctx, c, 1, 1, 2)
    try:
        d_V = dv.dev(V)[0]
        assert d_V.data_ptr() % 16 == 0 and V.size > 2048
        assert pb.set_photometric(None, d_V, v_min=v_min) == 0
        counts = pb.prepare(_images(c, 1, "sharp"), dv.dev_depth(c["depth"]), _images(c, 1, "blur"))
        ref0, cur0, _ = _level0(pb, counts)
        for got, which in ((ref0, "sharp"), (cur0, "blur")):
            _same(got, [pc.remap(c["raw"][which][b], maps[cal[b]], identity, inv[cal[b]]) for b in range(B)], ("raw", which, v_min))
    finally:
        pb.close()


def test_plain_load_variants_on_the_larger_shapes_in_a_child_process(mbavo, gpu_ctx):
    """MBAVO_PAIRS_PHOTOCAL_LDS=0 (see test_plain_load_variants_in_a_child_process): object B's calibrated entries and the 64 x 80
    pinhole camera set under the kernels that read the table by plain loads."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MBAVO_PAIRS_PHOTOCAL_LDS="0")
    pick = "test_every_entry_equals_the_calibrated_restatement[B] or test_pinhole_camera_set_over_two_workgroups[64-80]"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_pairs_photocal_options.py"), os.path.abspath(__file__), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider", "-k", pick], env=env, capture_output=True, text=True, timeout=120, cwd=os.path.dirname(here))
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
