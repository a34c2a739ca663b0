"""Caller-supplied masks on the device (mbavo_pairs_opts.mask, mbavo_pairs_set_masks, mbavo_undistort_mask_batch,
mbavo_mask_clearance_batch): a bonnet, a strut, a segmentation -- beside the clearance mask.

The stand-alone entries are held byte for byte to numpy (tests/pairs_mask_ref.py on top of tests/pairs_valid_ref.py).  The
object is held to what exists: an object with mask = 1 and masks set against the same object with mask = 0 and valid_radius = 0,
whose keypoint lists filtered by the numpy pyramid of (map, mask) -- in order -- are what it must hold, with identical images,
gradients and call statistics; a camera set against one-pair objects; an update against a fresh prepare.  Every comparison is exact.

Shapes are those of the clearance tests (tests/test_gpu_pairs_valid.py): 50 x 70 from a 60 x 80 raw camera, L = 3, B = 3 -- W no
multiple of 4, last rows and columns in no box, packed levels off a word; 45 x 63, where H W is odd and the second mask and map of
a batch start off a word; 100 x 140 with L = 6 for the coarse launch.  tests/test_pairs_mask_api.py asserts on the CPU that the
bonnet drops at least 10 % and keeps at least 25 % of what the clearance mask alone keeps."""
import numpy as np
import pytest

import lm_support as lms
import pairs_cases as cases
import pairs_device as dv
import pairs_mask_ref as mref
import pairs_step as ps
import pairs_valid_ref as vref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
B, L, H, W, HS, WS = 3, vref.L, vref.H, vref.W, vref.HS, vref.WS
CELL, THR, BORDERS = 6, 3.0, (3, 2, 1)
DEPTH = {0: dict(depth_format=0, depth_unit=0.0, depth_max=0.0), 2: dict(depth_format=2, depth_unit=5000.0, depth_max=0.0)}
NAMES = ("radtan", "unified")
IDX = [1, 0, 1]

_CASE = {}


def _case():
    """Everything numpy, made once and left unchanged: the case of the clearance tests (maps, raw images, depth maps), the raw masks
    and their numpy warps through both maps, and pinhole 50 x 70 images and depth maps for the objects without a map."""
    if not _CASE:
        c = cases.valid_case()
        hand, _ = vref.handcrafted_map()
        raw = {n: f() for n, f in mref.MASKS.items()}
        maps = dict(c["maps"], handcrafted=hand)
        tex = lambda seed: np.stack([synth.texture_image(H, W, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        _CASE.update(c, all_maps=maps, raw_masks=raw, warped={(k, n): mref.warp_mask(raw[k], m) for k in raw for n, m in maps.items()},
                     pin_sharp=tex(11), pin_blur=tex(111), pin_depth={0: cases.raw_depth(0, B, H, W, seed=33), 2: cases.raw_depth(2, B, H, W, seed=43)})
    return _CASE


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_maps(ctx):
    """The three maps on the device: both cameras (the device's own, held to numpy's bits) and the handcrafted one."""
    import torch
    c = _case()
    dev = [cases.valid_device_map(ctx, n) for n in NAMES]
    for n, d in zip(NAMES, dev):
        assert dv.same_bits(d.cpu().numpy(), c["maps"][n]), n
    return torch.stack(dev + [_t(c["all_maps"]["handcrafted"])]).contiguous(), list(NAMES) + ["handcrafted"]


def _object(ctx, r, dense, undistort=1, name="radtan", fmt=0, pairs=B, num_cameras=0, mask=1, **kw):
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, pairs, L=L, H=H, W=W, intr=vref.CAMERAS[name]["to_intr"], border=list(BORDERS), cell=0 if dense else CELL,
                             thresh=THR, every_candidate=dense, undistort=undistort, num_cameras=num_cameras, valid_radius=r, mask=mask,
                             **dict(DEPTH[fmt], **kw))
    if num_cameras == 0 and undistort != 0:
        assert pb.set_camera(cases.valid_camera(name)) == 0
    return pb


def _inputs(c, undistort, fmt, which=""):
    """(sharp, depth, blur) numpy arrays for an object with this undistort: raw images (and, undistort = 2, raw depth) or pinhole."""
    if undistort == 0:
        return c["pin_sharp"], c["pin_depth"][fmt], c["pin_blur"]
    depth = c["new_depth" if which else "depth"]
    d = depth[fmt] if (undistort == 2) == (fmt == 2) else (cases.raw_depth(fmt, B, H, W, seed=57) if undistort == 1 else cases.raw_depth(fmt, B, HS, WS, seed=58))
    return c[which + "sharp"], d, c[which + "blur"]


def _prepare(pb, sharp, depth, blur, rows=None):
    sel = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[list(rows)]))
    return pb.prepare(dv.dev(sel(sharp))[0], dv.dev_depth(sel(depth)), dv.dev(sel(blur))[0])


# ---- check 1: the warp
def test_mask_warp_equals_numpy(mbavo, gpu_ctx):
    """n = 3 maps (both cameras and the handcrafted one), every test mask, byte for byte; three in one call equal three single
    calls; nothing is written around an output that starts 3 bytes off a word."""
    import torch
    from mba_vo_amd import workloads
    c = _case()
    maps, names = _device_maps(gpu_ctx)
    for k, raw in c["raw_masks"].items():
        got = workloads.undistort_mask(gpu_ctx, _t(np.stack([raw] * 3)), maps).cpu().numpy()
        assert got.shape == (3, H, W) and got.dtype == np.uint8
        for i, n in enumerate(names):
            assert np.array_equal(got[i], c["warped"][(k, n)]), (k, n, int((got[i] != c["warped"][(k, n)]).sum()))
            one = workloads.undistort_mask(gpu_ctx, _t(raw), maps[i].contiguous()).cpu().numpy()
            assert np.array_equal(one[0], got[i]), (k, n)
        assert got.min() == 0 and got.max() == 1
    kinds = sorted(c["raw_masks"])  # three different masks in one call: mask i goes through map i
    raws = _t(np.stack([c["raw_masks"][k] for k in kinds]))
    want = np.stack([c["warped"][(k, n)] for k, n in zip(kinds, names)])
    assert np.array_equal(workloads.undistort_mask(gpu_ctx, raws, maps).cpu().numpy(), want)
    npx = H * W
    buf = torch.full((3 * npx + 8,), 7, dtype=torch.uint8, device="cuda:0")
    assert gpu_ctx.lib.mbavo_undistort_mask_batch(gpu_ctx.handle, 3, raws.data_ptr(), HS, WS, maps.data_ptr(), H, W, buf.data_ptr() + 3) == 0
    out = buf.cpu().numpy()
    assert np.all(out[:3] == 7) and np.all(out[3 + 3 * npx:] == 7)
    assert np.array_equal(out[3:3 + 3 * npx].reshape(3, H, W), want)


def test_mask_warp_and_clearance_where_h_w_is_odd(mbavo, gpu_ctx):
    """45 x 63: the second map starts 8 bytes off a 16-byte boundary and the second mask off a word -- the byte branches."""
    from mba_vo_amd import workloads
    c = _case()
    h, w = 45, 63
    maps = np.stack([vref.camera_map(vref.CAMERAS[n], h, w) for n in NAMES])
    raws = np.stack([c["raw_masks"]["bonnet"], c["raw_masks"]["scatter"]])
    want = np.stack([mref.warp_mask(raws[i], maps[i]) for i in range(2)])
    assert (h * w) % 2 == 1 and want.min() == 0 and want.max() == 1
    dm = _t(maps)
    got = workloads.undistort_mask(gpu_ctx, _t(raws), dm)
    assert np.array_equal(got.cpu().numpy(), want)
    for r in (0, 1):
        ref = np.stack([vref.packed(mref.clearance(maps[i], want[i], L, r)) for i in range(2)])
        assert np.array_equal(workloads.mask_clearance(gpu_ctx, dm, got, HS, WS, L, r).cpu().numpy(), ref), r
        ref = np.stack([vref.packed(mref.clearance(None, want[i], L, r)) for i in range(2)])
        assert np.array_equal(workloads.mask_clearance(gpu_ctx, None, got, 0, 0, L, r).cpu().numpy(), ref), r


def test_mask_warp_rejects_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    import torch
    lib = gpu_ctx.lib
    c = _case()
    m, raw = _t(c["maps"]["radtan"]), _t(c["raw_masks"]["bonnet"])
    out = torch.full((H * W,), 7, dtype=torch.uint8, device="cuda:0")
    mp, rp, op = m.data_ptr(), raw.data_ptr(), out.data_ptr()
    for args in ((1, None, HS, WS, mp, H, W, op), (1, rp, HS, WS, None, H, W, op), (1, rp, HS, WS, mp, H, W, None), (0, rp, HS, WS, mp, H, W, op),
                 (-1, rp, HS, WS, mp, H, W, op), (65536, rp, HS, WS, mp, H, W, op), (1, rp, 0, WS, mp, H, W, op), (1, rp, HS, -2, mp, H, W, op),
                 (1, rp, 2049, 2048, mp, H, W, op), (1, rp, HS, WS, mp, 0, W, op), (1, rp, HS, WS, mp, H, -1, op), (1, rp, HS, WS, mp, 2048, 2049, op)):
        assert lib.mbavo_undistort_mask_batch(gpu_ctx.handle, *args) == E_ARG, args
    assert lib.mbavo_undistort_mask_batch(None, 1, rp, HS, WS, mp, H, W, op) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- check 2: the pyramid of map and mask
def test_mask_clearance_equals_numpy(mbavo, gpu_ctx):
    """r = 0, 1, 3, 8 in three forms: map only (also the bytes of mbavo_undistort_clearance_batch), mask only, map and mask."""
    from mba_vo_amd import workloads
    c = _case()
    maps, names = _device_maps(gpu_ctx)
    np_maps = [c["all_maps"][n] for n in names]
    kinds = sorted(c["raw_masks"])
    masks = np.stack([c["warped"][(k, n)] * np.uint8(1 + 84 * i) for i, (k, n) in enumerate(zip(kinds, names))])  # (usable bytes: 1, 85, 169)
    dmasks = _t(masks)
    nbytes = vref.pyramid_bytes(H, W, L)
    for r in (0, 1, 3, 8):
        only_map = workloads.mask_clearance(gpu_ctx, maps, None, HS, WS, L, r).cpu().numpy()
        assert np.array_equal(only_map, workloads.undistort_clearance(gpu_ctx, maps, HS, WS, L, r).cpu().numpy()), r
        only_mask = workloads.mask_clearance(gpu_ctx, None, dmasks, -5, 0, L, r).cpu().numpy()  # (no map: Hs, Ws are not read)
        both = workloads.mask_clearance(gpu_ctx, maps, dmasks, HS, WS, L, r).cpu().numpy()
        for i in range(3):
            for got, ref, tag in ((only_map, mref.clearance(np_maps[i], None, L, r), "map"), (only_mask, mref.clearance(None, masks[i], L, r), "mask"),
                                  (both, mref.clearance(np_maps[i], masks[i], L, r), "both")):
                assert got.shape == (3, nbytes) and np.array_equal(got[i], vref.packed(ref)), (r, i, tag, int((got[i] != vref.packed(ref)).sum()))
            one = workloads.mask_clearance(gpu_ctx, maps[i].contiguous(), dmasks[i].contiguous(), HS, WS, L, r).cpu().numpy()
            assert np.array_equal(one[0], both[i]), (r, i)
        assert r == 8 or (both[:, :H * W].max() == 1 and both[:, :H * W].min() == 0)


def test_mask_clearance_reaches_past_three_levels(mbavo, gpu_ctx):
    """L = 6 at 100 x 140, r = 0 and 1, the three forms."""
    from mba_vo_amd import workloads
    h, w, levels = 100, 140, 6
    cam = vref.CAMERAS["radtan"]
    to = (2 * cam["to_intr"][0], 2 * cam["to_intr"][1], (w - 1) / 2 + 0.3, (h - 1) / 2 - 0.2)
    m = vref.cref.maps_of([dict(cam, to_intr=to)], h, w)[0]
    mask = mref.bonnet(h, w, height=0.2, half_width=0.4)  # (low enough to leave boxes of 32 x 32 valid)
    assert vref.valid_level(mref.valid0(m, mask), 5).any() and vref.valid_level(mref.valid0(None, mask), 5).any()
    assert not vref.valid_level(mref.valid0(None, mask), 5).all() and mref.valid0(m, mask).sum() < min(mref.valid0(m, None).sum(), (mask != 0).sum())
    dm, dk = _t(m), _t(mask)
    for r in (0, 1):
        for a, k, am, ak in ((dm, None, m, None), (None, dk, None, mask), (dm, dk, m, mask)):
            got = workloads.mask_clearance(gpu_ctx, a, k, HS, WS, levels, r).cpu().numpy()
            assert np.array_equal(got[0], vref.packed(mref.clearance(am, ak, levels, r))), (r, am is not None, ak is not None)


def test_mask_clearance_rejects_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    import torch
    lib = gpu_ctx.lib
    c = _case()
    m, k = _t(c["maps"]["radtan"]), _t(c["warped"][("bonnet", "radtan")])
    out = torch.full((vref.pyramid_bytes(H, W, L),), 7, dtype=torch.uint8, device="cuda:0")
    mp, kp, op = m.data_ptr(), k.data_ptr(), out.data_ptr()
    for args in ((1, None, None, H, W, HS, WS, L, 1, op), (1, mp, kp, H, W, HS, WS, L, 1, None), (0, mp, kp, H, W, HS, WS, L, 1, op),
                 (65536, mp, kp, H, W, HS, WS, L, 1, op), (1, mp, kp, H, W, HS, WS, 0, 1, op), (1, None, kp, H, W, HS, WS, 9, 1, op),
                 (1, mp, kp, 3, W, HS, WS, 3, 1, op), (1, None, kp, H, 3, HS, WS, 3, 1, op), (1, mp, kp, 2048, 2049, HS, WS, 1, 1, op),
                 (1, mp, kp, H, W, 0, WS, L, 1, op), (1, mp, None, H, W, HS, -2, L, 1, op), (1, mp, kp, H, W, 2049, 2048, L, 1, op),
                 (1, mp, kp, H, W, HS, WS, L, -1, op), (1, None, kp, H, W, HS, WS, L, 65, op)):
        assert lib.mbavo_mask_clearance_batch(gpu_ctx.handle, *args) == E_ARG, args
    assert lib.mbavo_mask_clearance_batch(None, 1, mp, kp, H, W, HS, WS, L, 1, op) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- check 3: the masked object against the unmasked one
@pytest.mark.parametrize("undistort,r,fmt", [(0, 0, 0), (0, 2, 2), (1, 2, 0), (2, 2, 2)])
@pytest.mark.parametrize("dense", [False, True])
def test_masked_batch_is_the_unmasked_batch_filtered(mbavo, gpu_ctx, undistort, r, fmt, dense):
    """mask = 1 with the bonnet set (undistort = 0: drawn in the image, geometry 0; else the raw bonnet, geometry 1) against mask = 0,
    valid_radius = 0: the lists filtered by the numpy pyramid of (map or none, mask) at radius r, in order; images, gradients and
    the launch / synchronisation / D2H statistics identical; keypoints dropped and kept at level 0."""
    c = _case()
    sharp, depth, blur = _inputs(c, undistort, fmt)
    if undistort == 0:
        mask, geometry, clear = mref.bonnet_undistorted(), 0, mref.clearance(None, mref.bonnet_undistorted(), L, r)
    else:
        mask, geometry, clear = c["raw_masks"]["bonnet"], 1, mref.clearance(c["maps"]["radtan"], c["warped"][("bonnet", "radtan")], L, r)
    plain = _object(gpu_ctx, 0, dense, undistort=undistort, fmt=fmt, mask=0)
    pb = _object(gpu_ctx, r, dense, undistort=undistort, fmt=fmt)
    try:
        base = dv.read_batch(plain, _prepare(plain, sharp, depth, blur))
        assert pb.set_masks(_t(mask[None]), geometry) == 0
        counts = _prepare(pb, sharp, depth, blur)
        want, dropped, kept = cases.filtered(base, [clear] * B)
        print("undistort %d r %d dense %s: level-0 keypoints dropped %d kept %d" % (undistort, r, dense, dropped, kept))
        assert dropped > 0 and kept > 0
        assert np.array_equal(counts, cases.counts_of(want))
        dv.assert_twins(dv.read_batch(pb, counts), want, (undistort, r, fmt, dense))
        assert pb.stats()[:3] == plain.stats()[:3] and pb.stats()[3] > plain.stats()[3]
    finally:
        pb.close()
        plain.close()


# ---- check 4: no mask set yet
@pytest.mark.parametrize("dense", [False, True])
def test_before_the_first_set_masks_the_object_is_the_clearance_object(mbavo, gpu_ctx, dense):
    c = _case()
    sharp, depth, blur = _inputs(c, 1, 0)
    pb, only = _object(gpu_ctx, 2, dense), _object(gpu_ctx, 2, dense, mask=0)
    try:
        counts, oc = _prepare(pb, sharp, depth, blur), _prepare(only, sharp, depth, blur)
        assert np.array_equal(counts, oc)
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(only, oc), dense)
        assert pb.stats()[:3] == only.stats()[:3]
    finally:
        pb.close()
        only.close()


# ---- check 5: the two geometries, and what set_masks rejects
def test_raw_geometry_masks_equal_their_numpy_warp_in_the_undistorted_geometry(mbavo, gpu_ctx):
    c = _case()
    sharp, depth, blur = _inputs(c, 1, 0)
    a, b = _object(gpu_ctx, 1, True, name="unified"), _object(gpu_ctx, 1, True, name="unified")
    try:
        assert a.set_masks(_t(c["raw_masks"]["scatter"][None]), 1) == 0
        assert b.set_masks(_t((c["warped"][("scatter", "unified")] * np.uint8(200))[None]), 0) == 0
        ca, cb = _prepare(a, sharp, depth, blur), _prepare(b, sharp, depth, blur)
        assert np.array_equal(ca, cb)
        dv.assert_twins(dv.read_batch(a, ca), dv.read_batch(b, cb), "geometry")
        plain = _object(gpu_ctx, 0, True, name="unified", mask=0)
        try:
            want, dropped, kept = cases.filtered(dv.read_batch(plain, _prepare(plain, sharp, depth, blur)),
                                                 [mref.clearance(c["maps"]["unified"], c["warped"][("scatter", "unified")], L, 1)] * B)
            assert dropped > 0 and kept > 0
            dv.assert_twins(dv.read_batch(a, ca), want, "geometry, numpy")
        finally:
            plain.close()
    finally:
        a.close()
        b.close()


def test_set_masks_rejects_what_the_header_says(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    c = _case()
    lib = gpu_ctx.lib
    und, raw = _t(np.stack([mref.bonnet_undistorted()] * 3)), _t(np.stack([c["raw_masks"]["bonnet"]] * 3))
    sharp, depth, blur = _inputs(c, 1, 0)
    off = _object(gpu_ctx, 2, False, mask=0)
    one = _object(gpu_ctx, 2, False)
    pin = _object(gpu_ctx, 2, False, undistort=0)
    cams = workloads.PairBatch(gpu_ctx, B, L=L, H=H, W=W, border=list(BORDERS), cell=CELL, thresh=THR, undistort=1, num_cameras=2, valid_radius=1, mask=1)
    try:
        before = _prepare(one, sharp, depth, blur)
        assert lib.mbavo_pairs_set_masks(off.handle, 0, 1, und.data_ptr()) == E_ARG          # opts.mask == 0
        for geometry, n, ptr in ((0, 2, und.data_ptr()), (0, 0, und.data_ptr()), (0, 1, None), (2, 1, und.data_ptr()), (-1, 1, und.data_ptr()),
                                 (1, 3, raw.data_ptr())):
            assert lib.mbavo_pairs_set_masks(one.handle, geometry, n, ptr) == E_ARG, (geometry, n)
        assert lib.mbavo_pairs_set_masks(pin.handle, 1, 1, raw.data_ptr()) == E_ARG          # geometry 1 with undistort == 0
        assert lib.mbavo_pairs_set_masks(pin.handle, 0, 1, und.data_ptr()) == 0
        assert lib.mbavo_pairs_set_masks(cams.handle, 1, 2, raw.data_ptr()) == E_ARG         # geometry 1 before the first camera call
        assert lib.mbavo_pairs_set_masks(cams.handle, 0, 1, und.data_ptr()) == E_ARG         # n != G'
        assert lib.mbavo_pairs_set_masks(cams.handle, 0, 2, und.data_ptr()) == 0             # geometry 0 needs no camera
        assert np.array_equal(_prepare(one, sharp, depth, blur), before)                     # nothing was changed by the rejected calls
    finally:
        for pb in (off, one, pin, cams):
            pb.close()


# ---- check 6: a set of cameras, every camera with its own mask
@pytest.mark.parametrize("G,undistort,fmt,dense", [(2, 1, 0, False), (2, 2, 2, True), (3, 1, 0, True), (3, 2, 2, False)])
def test_every_pair_is_filtered_by_its_own_cameras_mask(mbavo, gpu_ctx, G, undistort, fmt, dense):
    """G = 2: cameras (radtan, unified) with masks (bonnet, scatter), pair -> camera [1, 0, 1].  G = B = 3: one camera and one mask
    per pair (radtan, unified, radtan with bonnet, scatter, planted).  The object equals three one-pair objects built with the
    pair's camera and mask."""
    from mba_vo_amd import workloads
    c = _case()
    sharp, depth, blur = _inputs(c, undistort, fmt)
    names, idx = (list(NAMES), IDX) if G == 2 else (["radtan", "unified", "radtan"], [0, 1, 2])
    kinds = ["bonnet", "scatter", "planted"][:G]
    cams = [workloads.pairs_camera(cases.valid_camera(n), vref.CAMERAS[n]["to_intr"]) for n in names]
    raws = _t(np.stack([c["raw_masks"][k] for k in kinds]))
    multi = _object(gpu_ctx, 1, dense, undistort=undistort, fmt=fmt, num_cameras=G)
    singles = [_object(gpu_ctx, 1, dense, name=names[g], undistort=undistort, fmt=fmt, pairs=1) for g in idx]
    try:
        assert multi.set_cameras(cams, idx) == 0 and multi.set_masks(raws, 1) == 0
        counts = _prepare(multi, sharp, depth, blur)
        got = dv.read_batch(multi, counts)
        for b, pb in enumerate(singles):
            assert pb.set_masks(_t(c["raw_masks"][kinds[idx[b]]][None]), 1) == 0
            cb = _prepare(pb, sharp, depth, blur, rows=[b])
            assert np.array_equal(counts[b], cb[0]), (b, counts[b], cb)
            dv.assert_twins(got[b * L:(b + 1) * L], dv.read_batch(pb, cb), b)
        assert len({counts[b].tobytes() for b in range(B)}) > 1
    finally:
        for pb in [multi] + singles:
            pb.close()


# ---- check 7: a mask changed between two frames
@pytest.mark.parametrize("dense", [False, True])
def test_update_follows_the_new_mask_for_the_listed_pairs_only(mbavo, gpu_ctx, dense):
    c = _case()
    pb, fresh = _object(gpu_ctx, 1, dense), _object(gpu_ctx, 1, dense)
    try:
        assert pb.set_masks(_t(c["raw_masks"]["bonnet"][None]), 1) == 0
        first = dv.read_batch(pb, _prepare(pb, c["sharp"], c["depth"][0], c["blur"]))
        assert pb.set_masks(_t(c["raw_masks"]["scatter"][None]), 1) == 0
        keys = [0, 2]
        counts = pb.update(dv.dev(c["new_blur"])[0], keys, dv.dev(np.ascontiguousarray(c["new_sharp"][keys]))[0],
                           dv.dev_depth(np.ascontiguousarray(c["new_depth"][0][keys])))
        got = dv.read_batch(pb, counts)
        sharp, depth = c["sharp"].copy(), c["depth"][0].copy()
        sharp[keys], depth[keys] = c["new_sharp"][keys], c["new_depth"][0][keys]
        assert fresh.set_masks(_t(c["raw_masks"]["scatter"][None]), 1) == 0
        fc = _prepare(fresh, sharp, depth, c["new_blur"])
        want = dv.read_batch(fresh, fc)
        for b in keys:  # listed: a fresh prepare under the new mask
            assert np.array_equal(counts[b], fc[b])
            dv.assert_twins(got[b * L:(b + 1) * L], want[b * L:(b + 1) * L], ("listed", b))
        for e in range(1 * L, 2 * L):  # not listed: the keypoints it had, under the old mask
            assert dv.same_bits(got[e]["xy"], first[e]["xy"]) and dv.same_bits(got[e]["z"], first[e]["z"]) and dv.same_bits(got[e]["ref"], first[e]["ref"])
        assert not np.array_equal(counts[1], fc[1])  # (the two masks keep different keypoints of that pair)
    finally:
        pb.close()
        fresh.close()


# ---- check 8: a camera call keeps the stored mask
def test_a_camera_call_keeps_the_stored_mask_and_rebuilds_the_pyramid(mbavo, gpu_ctx):
    """Every candidate, r = 1: the keypoints show the whole pyramid.  A mask in the undistorted geometry, then the other raw camera
    (twice): the pyramid is numpy(new map, the same mask)."""
    from mba_vo_amd import workloads
    c = _case()
    sharp, depth, blur = _inputs(c, 1, 0)
    mask = mref.bonnet_undistorted()
    pb, plain = _object(gpu_ctx, 1, True), _object(gpu_ctx, 0, True, mask=0)
    try:
        assert pb.set_masks(_t(mask[None]), 0) == 0
        for _ in range(2):
            assert pb.set_camera(cases.valid_camera("unified")) == 0
        assert plain.set_camera(cases.valid_camera("unified")) == 0
        m = workloads.undistort_map(gpu_ctx, cases.valid_camera("unified"), vref.CAMERAS["radtan"]["to_intr"], H, W).cpu().numpy()
        clear = mref.clearance(m, mask, L, 1)
        assert not np.array_equal(clear[0], mref.clearance(c["maps"]["radtan"], mask, L, 1)[0]) and not np.array_equal(clear[0], mref.clearance(m, None, L, 1)[0])
        counts = _prepare(pb, sharp, depth, blur)
        want, dropped, kept = cases.filtered(dv.read_batch(plain, _prepare(plain, sharp, depth, blur)), [clear] * B)
        assert dropped > 0 and kept > 0
        dv.assert_twins(dv.read_batch(pb, counts), want, "camera call")
    finally:
        pb.close()
        plain.close()


# ---- check 9: a tracked frame
@pytest.mark.parametrize("undistort", [0, 1])
def test_a_tracked_frame_costs_what_it_costs_without_masks(mbavo, gpu_ctx, undistort):
    capi = mbavo.capi
    c = _case()
    sharp, depth, blur = _inputs(c, undistort, 0)
    kw = dict(S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
    pb, plain = _object(gpu_ctx, 2, False, undistort=undistort, **kw), _object(gpu_ctx, 0, False, undistort=undistort, mask=0, **kw)
    try:
        mask = mref.bonnet_undistorted() if undistort == 0 else c["raw_masks"]["bonnet"]
        assert pb.set_masks(_t(mask[None]), 0 if undistort == 0 else 1) == 0
        seen = []
        for o in (pb, plain):
            c0 = _prepare(o, sharp, depth, blur)
            assert o.set_states(o.initial_states(0.0, 0.1)) == 0
            keys = [0, 2]
            out, counts, _, _ = o.track_frame(dv.dev(blur)[0], np.full(B, 0.1), np.full(B, 0.02), lms.lm_batch_opts(capi, 2, 3), (ps.FLOW0, ps.FLOW1, ps.KERNEL),
                                              keys, dv.dev(np.ascontiguousarray(sharp[keys]))[0], dv.dev_depth(np.ascontiguousarray(depth[keys])))
            assert np.array_equal(counts, c0) and all(out[b].a.status == 0 and out[b].a.num_keypoints0 == c0[b, 0] for b in range(B))
            seen.append((o.stats()[:3], o.step_stats(), o.track_stats(), c0))
        assert seen[0][:3] == seen[1][:3], seen
        assert (seen[0][3] <= seen[1][3]).all() and seen[0][3][:, 0].sum() < seen[1][3][:, 0].sum()
    finally:
        pb.close()
        plain.close()
