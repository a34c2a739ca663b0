"""The clearance mask on the device (mbavo_pairs_opts.valid_radius, mbavo_undistort_clearance_batch): keypoints off the black
margin of undistorted images.

The stand-alone entry is held byte for byte to numpy (tests/pairs_valid_ref.py) on the maps read back from the device.  The
object is held to what exists: an object with valid_radius = r against the same object with valid_radius = 0, whose keypoint
lists filtered by the numpy clearance -- in order -- are what the r > 0 object must hold, with identical images, gradients and
call statistics; a camera set against one-pair objects; an update against a fresh prepare.  Every comparison is exact.

Shapes: 50 x 70 from a 60 x 80 raw camera, L = 3, B = 3: boxes that leave out the last rows and columns, a coarsest level of
12 x 17 that r = 8 empties, levels that start off a word in the packed layout.  The two cameras leave at r = 1 at least a quarter
of the inner pixels clear and a tenth not (tests/test_pairs_valid_api.py asserts it on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_cases as cases
import pairs_device as dv
import pairs_step as ps
import pairs_valid_ref as vref

pytestmark = pytest.mark.gpu

E_ARG = -1
B, L, H, W, HS, WS = cases.VALID_B, vref.L, vref.H, vref.W, vref.HS, vref.WS
CELL, THR, BORDERS = 6, 3.0, (3, 2, 1)
DEPTH = {0: dict(depth_format=0, depth_unit=0.0, depth_max=0.0), 2: dict(depth_format=2, depth_unit=5000.0, depth_max=0.0)}
NAMES = cases.VALID_NAMES
IDX = [1, 0, 1]  # the camera of every pair in the set (radtan, unified)


def _clear_of(name, r):
    return vref.clearance(cases.valid_case()["valid0"][name], L, r)


def _object(ctx, r, dense, name="radtan", undistort=1, fmt=0, pairs=B, num_cameras=0, **kw):
    """An object looking through camera `name` (num_cameras = 0: set here) or through a set (the caller sets it)."""
    from mba_vo_amd import workloads
    pb = workloads.PairBatch(ctx, pairs, L=L, H=H, W=W, intr=vref.CAMERAS[name]["to_intr"], border=list(BORDERS), cell=0 if dense else CELL,
                             thresh=THR, every_candidate=dense, undistort=undistort, num_cameras=num_cameras, valid_radius=r,
                             **dict(DEPTH[fmt], **kw))
    if num_cameras == 0:
        assert pb.set_camera(cases.valid_camera(name)) == 0
    return pb


def _prepare(pb, c, fmt=0, which="", rows=None):
    sel = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[list(rows)]))
    depth = c["new_depth" if which else "depth"][fmt]
    return pb.prepare(dv.dev(sel(c[which + "sharp"]))[0], dv.dev_depth(sel(depth)), dv.dev(sel(c[which + "blur"]))[0])


# ---- check 1: the stand-alone entry
def test_clearance_batch_equals_numpy(mbavo, gpu_ctx):
    """n = 3 maps (both cameras and the handcrafted one: NaN, +-inf, -0.0, the limits and their neighbours, 2^31) at r = 0, 1, 3, 8,
    byte for byte; three maps in one call equal three single calls; nothing is written around the output."""
    import torch
    from mba_vo_amd import workloads
    c = cases.valid_case()
    hand, want = vref.handcrafted_map()
    dev = [cases.valid_device_map(gpu_ctx, n) for n in NAMES]
    for n, d in zip(NAMES, dev):
        assert dv.same_bits(d.cpu().numpy(), c["maps"][n]), n  # (the numpy clearance below is that of the device's map)
    maps = torch.stack(dev + [torch.from_numpy(hand).to("cuda:0")]).contiguous()
    valid = [c["valid0"][n] for n in NAMES] + [vref.valid0(hand, HS, WS)]
    assert all(bool(valid[2][rc]) == ok for rc, ok in want.items())
    nbytes = vref.pyramid_bytes(H, W, L)
    assert gpu_ctx.lib.mbavo_undistort_clearance_bytes(H, W, L) == nbytes and nbytes % 4 != 0  # (the second map starts off a word)
    for r in (0, 1, 3, 8):
        got = workloads.undistort_clearance(gpu_ctx, maps, HS, WS, L, r).cpu().numpy()
        assert got.shape == (3, nbytes) and got.dtype == np.uint8
        for i in range(3):
            ref = vref.packed(vref.clearance(valid[i], L, r))
            assert np.array_equal(got[i], ref), (r, i, int((got[i] != ref).sum()))
            one = workloads.undistort_clearance(gpu_ctx, maps[i].contiguous(), HS, WS, L, r).cpu().numpy()
            assert np.array_equal(one[0], got[i]), (r, i)
            lv = workloads.clearance_levels(got[i], H, W, L)
            assert r < 8 or not lv[2].any()
        assert got[:2, :H * W].min() == 0 and (r == 8 or got[:2, :H * W].max() == 1)
    buf = torch.full((3 * nbytes + 8,), 7, dtype=torch.uint8, device="cuda:0")
    assert gpu_ctx.lib.mbavo_undistort_clearance_batch(gpu_ctx.handle, 3, maps.data_ptr(), H, W, HS, WS, L, 1, buf.data_ptr() + 3) == 0
    out = buf.cpu().numpy()
    assert np.all(out[:3] == 7) and np.all(out[3 + 3 * nbytes:] == 7)
    assert np.array_equal(out[3:3 + 3 * nbytes].reshape(3, nbytes), workloads.undistort_clearance(gpu_ctx, maps, HS, WS, L, 1).cpu().numpy())


def test_clearance_batch_reaches_past_three_levels(mbavo, gpu_ctx):
    """L = 6 at 100 x 140 (levels 4 and 5 come from level 3 in a launch of their own; 3 x 4 pixels at the end), r = 0 and 1."""
    import torch
    from mba_vo_amd import workloads
    h, w, levels = 100, 140, 6
    cam = vref.CAMERAS["radtan"]
    to = (2 * cam["to_intr"][0], 2 * cam["to_intr"][1], (w - 1) / 2 + 0.3, (h - 1) / 2 - 0.2)
    m = vref.cref.maps_of([dict(cam, to_intr=to)], h, w)[0]
    v0 = vref.valid0(m, HS, WS)
    assert 0.5 < v0.mean() < 0.95 and vref.valid_level(v0, 5).any() and not vref.valid_level(v0, 5).all()
    for r in (0, 1):
        got = workloads.undistort_clearance(gpu_ctx, torch.from_numpy(m).to("cuda:0"), HS, WS, levels, r).cpu().numpy()
        assert np.array_equal(got[0], vref.packed(vref.clearance(v0, levels, r))), r


def test_clearance_batch_rejects_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    import torch
    lib = gpu_ctx.lib
    m = torch.from_numpy(cases.valid_case()["maps"]["radtan"]).to("cuda:0")
    out = torch.full((vref.pyramid_bytes(H, W, L),), 7, dtype=torch.uint8, device="cuda:0")
    mp, op = m.data_ptr(), out.data_ptr()
    for args in ((1, None, H, W, HS, WS, L, 1, op), (1, mp, H, W, HS, WS, L, 1, None), (0, mp, H, W, HS, WS, L, 1, op),
                 (-1, mp, H, W, HS, WS, L, 1, op), (65536, mp, H, W, HS, WS, L, 1, op), (1, mp, H, W, HS, WS, 0, 1, op),
                 (1, mp, H, W, HS, WS, 9, 1, op), (1, mp, 3, W, HS, WS, 3, 1, op), (1, mp, H, 3, HS, WS, 3, 1, op),
                 (1, mp, 0, W, HS, WS, 1, 1, op), (1, mp, H, -1, HS, WS, 1, 1, op), (1, mp, 2048, 2049, HS, WS, 1, 1, op),
                 (1, mp, H, W, 0, WS, L, 1, op), (1, mp, H, W, HS, -2, L, 1, op), (1, mp, H, W, 2049, 2048, L, 1, op),
                 (1, mp, H, W, HS, WS, L, -1, op), (1, mp, H, W, HS, WS, L, 65, op)):
        assert lib.mbavo_undistort_clearance_batch(gpu_ctx.handle, *args) == E_ARG, args
    assert lib.mbavo_undistort_clearance_batch(None, 1, mp, H, W, HS, WS, L, 1, op) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert lib.mbavo_undistort_clearance_batch(gpu_ctx.handle, 1, mp, H, W, HS, WS, L, 64, op) == 0  # the largest radius: nothing is clear
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---- checks 2 and 3: the batch against the unmasked batch
@pytest.mark.parametrize("dense", [False, True])
def test_masked_batch_is_the_unmasked_batch_filtered(mbavo, gpu_ctx, dense):
    """r = 1 and r = 3 against r = 0: counts and keypoints at every level are the r = 0 lists filtered by the numpy clearance of
    the map, in order; images, gradients and the launch / synchronisation / D2H statistics are identical; at level 0 keypoints are
    dropped and kept."""
    c = cases.valid_case()
    assert dv.same_bits(cases.valid_device_map(gpu_ctx, "radtan").cpu().numpy(), c["maps"]["radtan"])
    plain = _object(gpu_ctx, 0, dense)
    try:
        base = dv.read_batch(plain, _prepare(plain, c))
        stats0 = plain.stats()
        for r in (1, 3):
            pb = _object(gpu_ctx, r, dense)
            try:
                counts = _prepare(pb, c)
                want, dropped, kept = cases.filtered(base, [_clear_of("radtan", r)] * B)
                print("dense %s r %d: level-0 keypoints dropped %d kept %d" % (dense, r, dropped, kept))
                assert dropped > 0 and kept > 0
                assert np.array_equal(counts, cases.counts_of(want))
                dv.assert_twins(dv.read_batch(pb, counts), want, (dense, r))
                assert pb.stats()[:3] == stats0[:3] and pb.stats()[3] > stats0[3]
            finally:
                pb.close()
    finally:
        plain.close()


# ---- check 4: a set of cameras
@pytest.mark.parametrize("undistort,fmt", [(1, 0), (2, 2)])
@pytest.mark.parametrize("dense", [False, True])
def test_every_pair_is_filtered_by_its_own_camera(mbavo, gpu_ctx, undistort, fmt, dense):
    """num_cameras = 2 (one camera of each model), camera_of_pair = [1, 0, 1], r = 1: the object equals three one-pair objects built
    with the pair's camera and the same r, array for array, and the r = 0 set filtered by every pair's own clearance."""
    from mba_vo_amd import workloads
    c = cases.valid_case()
    cams = [workloads.pairs_camera(cases.valid_camera(n), vref.CAMERAS[n]["to_intr"]) for n in NAMES]
    multi, plain = (_object(gpu_ctx, r, dense, undistort=undistort, fmt=fmt, num_cameras=2) for r in (1, 0))
    singles = [_object(gpu_ctx, 1, dense, name=NAMES[g], undistort=undistort, fmt=fmt, pairs=1) for g in IDX]
    try:
        assert multi.set_cameras(cams, IDX) == 0 and plain.set_cameras(cams, IDX) == 0
        counts = _prepare(multi, c, fmt)
        got = dv.read_batch(multi, counts)
        for b, pb in enumerate(singles):
            cb = _prepare(pb, c, fmt, rows=[b])
            assert np.array_equal(counts[b], cb[0]), (b, counts[b], cb)
            dv.assert_twins(got[b * L:(b + 1) * L], dv.read_batch(pb, cb), b)
        want, dropped, kept = cases.filtered(dv.read_batch(plain, _prepare(plain, c, fmt)), [_clear_of(NAMES[g], 1) for g in IDX])
        assert dropped > 0 and kept > 0
        dv.assert_twins(got, want, "set")
        assert multi.stats()[:3] == plain.stats()[:3]
    finally:
        for pb in [multi, plain] + singles:
            pb.close()


# ---- check 5: update and camera change
@pytest.mark.parametrize("dense", [False, True])
def test_update_equals_a_fresh_prepare_and_a_new_camera_rebuilds_the_mask(mbavo, gpu_ctx, dense):
    c = cases.valid_case()
    from mba_vo_amd import workloads
    pb, fresh = _object(gpu_ctx, 1, dense), _object(gpu_ctx, 1, dense)
    try:
        _prepare(pb, c)
        before = pb.step_stats()[0]
        counts = pb.update(dv.dev(c["new_blur"])[0], [1], dv.dev(np.ascontiguousarray(c["new_sharp"][[1]]))[0],
                           dv.dev_depth(np.ascontiguousarray(c["new_depth"][0][[1]])))
        assert pb.step_stats()[0] != before
        sharp, depth = c["sharp"].copy(), c["depth"][0].copy()
        sharp[1], depth[1] = c["new_sharp"][1], c["new_depth"][0][1]
        fc = fresh.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(c["new_blur"])[0])
        assert np.array_equal(counts, fc)
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(fresh, fc), "update")
        # the other model on the same object (its `to` camera stays): the mask follows the new map
        assert pb.set_camera(cases.valid_camera("unified")) == 0
        counts = _prepare(pb, c)
        again = _object(gpu_ctx, 0, dense)  # the same `to` camera, unmasked, through the unified raw camera
        try:
            assert again.set_camera(cases.valid_camera("unified")) == 0
            m = workloads.undistort_map(gpu_ctx, cases.valid_camera("unified"), vref.CAMERAS["radtan"]["to_intr"], H, W).cpu().numpy()
            clear = vref.clearance(vref.valid0(m, HS, WS), L, 1)
            assert not np.array_equal(clear[0], _clear_of("radtan", 1)[0])
            want, dropped, kept = cases.filtered(dv.read_batch(again, _prepare(again, c)), [clear] * B)
            assert dropped > 0 and kept > 0
            dv.assert_twins(dv.read_batch(pb, counts), want, "camera change")
        finally:
            again.close()
    finally:
        pb.close()
        fresh.close()


# ---- check 6: a tracked frame
def test_tracked_frame_counts_are_the_filtered_counts(mbavo, gpu_ctx):
    capi = mbavo.capi
    c = cases.valid_case()
    kw = dict(S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
    pb, plain = _object(gpu_ctx, 1, False, **kw), _object(gpu_ctx, 0, False, **kw)
    try:
        want, dropped, kept = cases.filtered(dv.read_batch(plain, _prepare(plain, c)), [_clear_of("radtan", 1)] * B)
        c0 = _prepare(pb, c)
        assert np.array_equal(c0, cases.counts_of(want)) and dropped > 0 and kept > 0
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
        keys = [0, 2]
        out, counts, _, _ = pb.track_frame(dv.dev(c["blur"])[0], np.full(B, 0.1), np.full(B, 0.02), lms.lm_batch_opts(capi, 2, 3), (ps.FLOW0, ps.FLOW1, ps.KERNEL),
                                           keys, dv.dev(np.ascontiguousarray(c["sharp"][keys]))[0], dv.dev_depth(np.ascontiguousarray(c["depth"][0][keys])))
        assert np.array_equal(counts, c0)  # the first keyframes again, filtered again
        assert all(out[b].a.status == 0 and out[b].a.num_keypoints0 == cases.counts_of(want)[b, 0] for b in range(B))
    finally:
        pb.close()
        plain.close()


# ---- check 7: the default is untouched
@pytest.mark.parametrize("dense", [False, True])
def test_an_object_without_the_mask_holds_the_bytes_it_held(mbavo, gpu_ctx, dense):
    """valid_radius = 0: mbavo_pairs_last_stats out[3] is the plan written out here, array by array, without a clearance byte."""
    al = lambda v, a=256: (v + a - 1) // a * a
    pb = _object(gpu_ctx, 0, dense)
    try:
        px = [(H >> l) * (W >> l) for l in range(L)]
        img = al(sum(al(p, 16) for p in px))
        grad = al(sum(al(p, 16) for p in px) * 8)
        cap = px if dense else [((H >> l) // int(CELL / 1.414 ** l) + 1) * ((W >> l) // int(CELL / 1.414 ** l) + 1) for l in range(L)]  # FeatureDetectorBase.cpp:56-64
        kp = sum(3 * al(k, 2) for k in cap) * 8
        picks, segs = (0, sum((p + 255) // 256 for p in px)) if dense else (sum(cap), 0)
        N, P = pb.N, 8
        want = (al(2 * B * img) + al(B * grad) + al(B * kp) + al(B * picks * 16) + al(B * segs * 4) + al(B * L * 4) + al(B * L * 88) + al(B * L * 8)
                + al(L * 2 * P * 4) + al(8 * H * W) + al(B * (2 + 7 * N) * 8))
        o = pb.opts
        nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
        assert gpu_ctx.lib.mbavo_pairs_plan(C.byref(o), C.byref(nbytes), cells) == 0
        assert list(cells)[:L] == cap
        assert pb.stats()[3] == nbytes.value == want, (pb.stats()[3], nbytes.value, want)
    finally:
        pb.close()
