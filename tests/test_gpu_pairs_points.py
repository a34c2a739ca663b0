"""Keypoints and depths from the caller on the device (mbavo_pairs_prepare_points, _update_points, _track_frame_points), all
through the C ABI.  The arrays are held bit for bit to the numpy restatement of the header's rule (tests/pairs_points_ref.py, itself
held to hand-made cases on the CPU by tests/test_pairs_points_api.py); pyramids and gradient images to the detector prepare on the
same images; an update to a fresh prepare; the detector's own keypoints fed back give the detector's arrays and the same LM run.

Shapes: 72 x 96 with L = 3, B = 3, border (3, 2, 1) and lists of 0, 5 and 300 points (the last crosses the 256-point step of the
workgroup loop; the every-candidate capacity at level 2 is 432), on a grid object (cells 6 x 6, capacities 221 / 130 / 63) lists of
0, 5 and 63; 50 x 70 from the 60 x 80 raw cameras of the clearance tests for masks and the black margin."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_cases as cases
import pairs_device as dv
import pairs_mask_ref as mref
import pairs_points_ref as pref
import pairs_step as ps
import pairs_track as pt
import pairs_valid_ref as vref
import scenes
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -2
B, L, H, W = 3, 3, 72, 96
BORDERS = (3, 2, 1)
THRESHOLDS = (ps.FLOW0, ps.FLOW1, ps.KERNEL)
_CASE = {}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _images(n, h, w, seed):
    return np.ascontiguousarray(np.stack([synth.texture_image(h, w, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(n)]))


def _list(n, h, w, borders, seed):
    """n level-0 points: the edge cases of the restatement first, then points on both sides of every level's border band, two
    groups that share a level-2 pixel, then random ones -- whole, half and arbitrary coordinates, depths on both sides of 1e-2,
    every kept depth different (the order shows)."""
    rng = np.random.default_rng(seed)
    pts = [(x, y, z) for x, y, z, _ in pref.edge_points(h, w, borders)]
    for l, m in enumerate(borders):
        s, hl, wl = 1 << l, h >> l, w >> l
        for x in (m - 1, m, wl - m - 1, wl - m):
            pts.append((float(x * s), float((hl // 2) * s), 1.0))
        for y in (m - 1, m, hl - m - 1, hl - m):
            pts.append((float((wl // 2) * s), float(y * s), 1.0))
    pts += [(40.0, 20.0, 1.0), (41.0, 21.0, 1.0), (39.0, 19.0, 1.0), (42.0, 22.0, 1.0)]
    xy = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1)
    xy[::3] = np.floor(xy[::3])
    xy[1::6] = np.floor(xy[1::6]) + 0.5
    z = rng.uniform(0.5, 3.0, n)
    z[rng.uniform(0, 1, n) < 0.1] = 0.005
    k = min(n, len(pts))
    pick = list(range(k)) if n >= len(pts) else sorted(rng.choice(len(pts), k, replace=False).tolist())
    for i, j in enumerate(pick):
        xy[i], z[i] = pts[j][:2], pts[j][2] if pts[j][2] != 1.0 else 1.0 + 1e-3 * i
    return np.ascontiguousarray(xy), np.ascontiguousarray(z)


def _case():
    if not _CASE:
        _CASE.update(sharp=_images(B, H, W, 5), blur=_images(B, H, W, 105), new_sharp=_images(4, H, W, 45), new_blur=_images(4, H, W, 145),
                     lists={n: _list(n, H, W, BORDERS, 100 + n) for n in (0, 5, 63, 300)}, more={7: _list(7, H, W, BORDERS, 207)})
    return _CASE


def _object(ctx, dense=True, pairs=B, fmt=0, **kw):
    from mba_vo_amd import workloads
    kw = dict(dict(L=L, H=H, W=W, border=list(BORDERS), cell=0 if dense else 6, thresh=3.0, every_candidate=dense, keyframe_format=fmt), **kw)
    return workloads.PairBatch(ctx, pairs, **kw)


def _assert_keypoints(got, want, counts, want_counts, tag):
    assert np.array_equal(counts, want_counts), (tag, counts, want_counts)
    for e, (g, w) in enumerate(zip(got, want)):
        assert dv.same_bits(g["xy"], w["xy"]) and dv.same_bits(g["z"], w["z"]), (tag, e)


def _capacity(ctx, pb):
    nbytes, cells = C.c_longlong(0), (C.c_int * 8)()
    assert ctx.lib.mbavo_pairs_plan(C.byref(pb.opts), C.byref(nbytes), cells) == 0
    return min(cells[:pb.L]), nbytes.value


# ---- check 1: the arrays against the restatement
@pytest.mark.parametrize("dense,fmt", [(True, 0), (False, 0), (False, 1), (False, 2)])
def test_arrays_equal_the_restatement_bit_for_bit(mbavo, gpu_ctx, dense, fmt):
    c = _case()
    lengths = (0, 5, 300) if dense else (0, 5, 63)
    points = [c["lists"][n] for n in lengths]
    want, want_counts = pref.keypoints(points, L, H, W, BORDERS)
    assert all(0 < want_counts[2, l] < lengths[2] for l in range(L)) and (want_counts[0] == 0).all()
    pb, det = _object(gpu_ctx, dense, fmt=fmt), _object(gpu_ctx, dense, fmt=fmt)
    try:
        assert _capacity(gpu_ctx, pb)[0] == (432 if dense else 63)
        sharp, blur = dv.dev(c["sharp"], c["blur"])
        counts = pb.prepare_points(sharp, blur, points)
        got = dv.read_batch(pb, counts)  # (asserts K of every problem == counts)
        _assert_keypoints(got, want, counts, want_counts, (dense, fmt))
        depth = _t(np.full((B, H, W), 1.5, np.float32))
        base = dv.read_batch(det, det.prepare(sharp, depth, blur))
        for e, (g, w) in enumerate(zip(got, base)):  # pyramids and gradient images are the detector prepare's
            assert all(dv.same_bits(g[key], w[key]) for key in ("ref", "cur", "grad")), (dense, fmt, e)
        again = pb.prepare_points(sharp, blur, points)  # deterministic
        _assert_keypoints(dv.read_batch(pb, again), want, again, want_counts, "again")
    finally:
        pb.close()
        det.close()


# ---- check 2: round trip through the detector
@pytest.mark.parametrize("k", [4, 2])
def test_the_detectors_own_keypoints_come_back_unchanged(mbavo, gpu_ctx, k):
    capi = mbavo.capi
    n, h, w = 2, 50, 70
    scs = [scenes.Scene(H=h, W=w, S=4, F=1, k=k, K=10, seed=20 + b, margin=10) for b in range(n)]
    rng = np.random.default_rng(8)
    depth = rng.uniform(0.8, 3.0, (n, h, w)).astype(np.float32)
    depth[rng.uniform(0, 1, (n, h, w)) < 0.15] = 0.0
    sharp, blur = np.stack([s.ref for s in scs]), np.stack([s.cur[0] for s in scs])
    N = scs[0].N
    kw = dict(pairs=n, L=1, H=h, W=w, border=[4], S=4, k=k, N=N)
    det, pts = _object(gpu_ctx, False, **kw), _object(gpu_ctx, False, **kw)
    try:
        ds, db = dv.dev(np.ascontiguousarray(sharp), np.ascontiguousarray(blur))
        dc = det.prepare(ds, _t(depth), db)
        first = dv.read_batch(det, dc)
        assert (dc > 20).all()
        counts = pts.prepare_points(ds, db, [(g["xy"], g["z"]) for g in first])
        assert np.array_equal(counts, dc)
        dv.assert_twins(dv.read_batch(pts, counts), first, "round trip")
        runs = []
        for pb in (det, pts):
            assert pb.set_motion([s.cap[0] for s in scs], [s.exp[0] for s in scs], [s.t0 for s in scs], scs[0].dt,
                                 np.stack([s.knots_t for s in scs]), np.stack([s.knots_R for s in scs])) == 0
            fields, recs, _ = dv.run_lm(gpu_ctx, capi, n, 1, pb.array, k)
            runs.append((fields, recs, pb.knots()))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
        assert np.array_equal(runs[0][2][0], runs[1][2][0]) and np.array_equal(runs[0][2][1], runs[1][2][1])
        assert sum(len(r) for r in runs[0][1]) > 0
    finally:
        det.close()
        pts.close()


# ---- check 3: an update equals a fresh prepare
@pytest.mark.parametrize("dense", [True, False])
def test_update_points_equals_a_fresh_prepare_points(mbavo, gpu_ctx, dense):
    c = _case()
    n = 4
    big = 300 if dense else 63
    sharp0, blur0 = np.concatenate([c["sharp"], c["new_sharp"][:1]]), np.concatenate([c["blur"], c["new_blur"][:1]])
    lists0 = [c["lists"][5], c["lists"][big], c["lists"][0], c["more"][7]]
    keys = [1, 3]
    new_lists = [c["more"][7], (np.ascontiguousarray(c["lists"][big][0][::-1]), np.ascontiguousarray(c["lists"][big][1][::-1]))]
    pb, fresh = _object(gpu_ctx, dense, pairs=n), _object(gpu_ctx, dense, pairs=n)
    try:
        before = dv.read_batch(pb, pb.prepare_points(*dv.dev(sharp0, blur0), lists0))
        new_sharp = np.ascontiguousarray(c["new_sharp"][keys])
        counts = pb.update_points(dv.dev(c["new_blur"])[0], keys, dv.dev(new_sharp)[0], new_lists)
        got = dv.read_batch(pb, counts)
        latest_sharp, latest_lists = sharp0.copy(), list(lists0)
        for i, b in enumerate(keys):
            latest_sharp[b], latest_lists[b] = new_sharp[i], new_lists[i]
        fc = fresh.prepare_points(*dv.dev(latest_sharp, c["new_blur"]), latest_lists)
        assert np.array_equal(counts, fc)
        dv.assert_twins(got, dv.read_batch(fresh, fc), ("update", dense))
        for b in (0, 2):  # the keyframe side of the pairs not listed: the same bytes as before
            for e in range(b * L, (b + 1) * L):
                assert all(dv.same_bits(got[e][key], before[e][key]) for key in ("ref", "grad", "xy", "z")), e
        assert not dv.same_bits(got[L]["xy"], before[L]["xy"]) and not dv.same_bits(got[L]["ref"], before[L]["ref"])  # (the listed pairs did change)
        # a detector update on pair 0 only: pair 0 holds detected keypoints, pairs 1 .. 3 still hold their points
        depth = _t(np.full((1, H, W), 2.5, np.float32))
        dcounts = pb.update(None, [0], dv.dev(np.ascontiguousarray(c["new_sharp"][2:3]))[0], depth)
        mixed = dv.read_batch(pb, dcounts)
        for e in range(L, n * L):
            assert all(dv.same_bits(mixed[e][key], got[e][key]) for key in ("ref", "cur", "grad", "xy", "z")), e
        assert np.array_equal(dcounts[1:], counts[1:]) and dcounts[0, 0] > 5 and np.all(mixed[0]["z"] == 2.5)
        ref = _object(gpu_ctx, dense, pairs=1)
        try:
            rc = ref.prepare(dv.dev(np.ascontiguousarray(c["new_sharp"][2:3]))[0], depth, dv.dev(np.ascontiguousarray(c["new_blur"][:1]))[0])
            assert np.array_equal(rc[0], dcounts[0])
            dv.assert_twins(mixed[:L], dv.read_batch(ref, rc), "detected pair")
        finally:
            ref.close()
        # n_key == 0: mbavo_pairs_update(d_blur, 0, ..) -- the point arguments are not read
        assert gpu_ctx.lib.mbavo_pairs_update_points(pb.handle, dv.dev(blur0)[0].data_ptr(), 0, None, None, None, None, None, None) == 0
        assert pb.step_stats()[0][1:] == (1, 0)
    finally:
        pb.close()
        fresh.close()


# ---- check 4: clearance and masks
def _rect_mask(h, w):
    m = np.full((h, w), 255, np.uint8)
    m[13:27, 21:38] = 0  # no edge on a multiple of 2 or 4
    return m


def test_points_are_tested_against_the_stored_mask(mbavo, gpu_ctx):
    """undistort = 0, mask = 1, valid_radius = 1 at 50 x 70: points inside the zero rectangle, next to it and far from it."""
    h, w = vref.H, vref.W
    mask = _rect_mask(h, w)
    clear = mref.clearance(None, mask, L, 1)
    ys, xs = np.mgrid[10:30:2, 18:42:2]  # in and around the rectangle (every list within the capacity of level 2: 12 x 17 = 204)
    near = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    far = _list(80, h, w, BORDERS, 9)[0]
    z = 1.0 + 1e-3 * np.arange(len(near) + len(far))
    points = [(np.concatenate([near, far]), z), (np.concatenate([far[::-1], near[::-1] + (0.5, -0.5)]), z[::-1].copy()), (np.concatenate([near[:40] + 1.0, far[:30]]), z[:70])]
    want, want_counts = pref.keypoints(points, L, h, w, BORDERS, [clear] * B)
    plain_counts = pref.keypoints(points, L, h, w, BORDERS)[1]
    assert (want_counts[:2] < plain_counts[:2]).all() and (want_counts > 0).all()
    pb = _object(gpu_ctx, True, H=h, W=w, mask=1, valid_radius=1)
    try:
        assert pb.set_masks(_t(mask[None]), 0) == 0
        counts = pb.prepare_points(*dv.dev(_images(B, h, w, 3), _images(B, h, w, 103)), points)
        _assert_keypoints(dv.read_batch(pb, counts), want, counts, want_counts, "mask")
    finally:
        pb.close()


@pytest.mark.parametrize("G", [0, 2])
def test_points_keep_off_the_black_margin_of_a_raw_camera(mbavo, gpu_ctx, G):
    """undistort = 1, valid_radius = 2: the radial-tangential camera of the clearance tests alone, and a set of two cameras (pairs
    -> unified, radtan, unified).  The level-0 images are the detector prepare's remap."""
    from mba_vo_amd import workloads
    c = cases.valid_case()
    h, w, r = vref.H, vref.W, 2
    names = ["radtan"] * B if G == 0 else ["unified", "radtan", "unified"]
    clears = {n: vref.clearance(c["valid0"][n], L, r) for n in set(names)}
    xy, z = _list(200, h, w, BORDERS, 17)  # (the capacity of level 2 is 12 x 17 = 204)
    ys, xs = np.mgrid[0:h:5, 0:w:5]
    grid = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    points = [(xy, z), (grid, 1.0 + 1e-3 * np.arange(len(grid))), (xy[::-1].copy(), z[::-1].copy())]
    want, want_counts = pref.keypoints(points, L, h, w, BORDERS, [clears[n] for n in names])
    assert (want_counts < pref.keypoints(points, L, h, w, BORDERS)[1]).any() and (want_counts[:, 0] > 0).all()
    kw = dict(H=h, W=w, undistort=1, valid_radius=r, num_cameras=G, intr=vref.CAMERAS["radtan"]["to_intr"])
    pb, det = _object(gpu_ctx, True, **kw), _object(gpu_ctx, True, **kw)
    try:
        for o in (pb, det):
            if G == 0:
                assert o.set_camera(cases.valid_camera("radtan")) == 0
            else:
                cams = [workloads.pairs_camera(cases.valid_camera(n), vref.CAMERAS[n]["to_intr"]) for n in ("radtan", "unified")]
                assert o.set_cameras(cams, [1, 0, 1]) == 0
        sharp, blur = dv.dev(c["sharp"], c["blur"])
        counts = pb.prepare_points(sharp, blur, points)
        got = dv.read_batch(pb, counts)
        _assert_keypoints(got, want, counts, want_counts, ("margin", G))
        base = dv.read_batch(det, det.prepare(sharp, _t(np.full((B, h, w), 1.5, np.float32)), blur))
        for e, (g, b_) in enumerate(zip(got, base)):
            assert all(dv.same_bits(g[key], b_[key]) for key in ("ref", "cur", "grad")), e
        assert pb.stats()[0] == det.stats()[0] - 2  # one points launch in place of count + scan + write
    finally:
        pb.close()
        det.close()


# ---- check 5: errors leave nothing behind
def test_errors_leave_nothing_behind(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    capi, lib = mbavo.capi, gpu_ctx.lib
    c = _case()
    sharp, blur = dv.dev(c["sharp"], c["blur"])
    points = [c["lists"][n] for n in (0, 5, 300)]
    pb = _object(gpu_ctx, True)
    cam = _object(gpu_ctx, True, H=vref.H, W=vref.W, undistort=1)
    try:
        off, xy, z = pb._point_lists(points, B)
        sp, bp, xp, zp = sharp.data_ptr(), blur.data_ptr(), xy.data_ptr(), z.data_ptr()
        ip = lambda a: capi.ip(np.ascontiguousarray(a, dtype=np.int32))
        # update_points before the first prepare
        assert lib.mbavo_pairs_update_points(pb.handle, bp, 1, ip([1]), sp, ip([0, 5]), xp, zp, None) == E_ARG
        assert pb.stats()[:3] == (0, 0, 0) and pb.step_stats()[0] == (0, 0, 0)
        good = pb.prepare_points(sharp, blur, points)
        held, stats = dv.read_batch(pb, good), pb.stats()
        cap = _capacity(gpu_ctx, pb)[0]
        assert cap == 432
        bad = [((None, bp, ip(off), xp, zp), E_ARG), ((sp, None, ip(off), xp, zp), E_ARG), ((sp, bp, None, xp, zp), E_ARG),
               ((sp, bp, ip(off), None, zp), E_ARG), ((sp, bp, ip(off), xp, None), E_ARG),
               ((sp, bp, ip([0, 5, 3, 305]), xp, zp), E_ARG),        # decreasing
               ((sp, bp, ip([1, 1, 6, 305]), xp, zp), E_ARG),        # does not start at 0
               ((sp, bp, ip([0, 0, 0, cap + 1]), xp, zp), E_RANGE)]  # one longer than the smallest capacity
        for args, want in bad:
            counts = np.full((B, L), -7, np.int32)
            assert lib.mbavo_pairs_prepare_points(pb.handle, *args, capi.ip(counts)) == want, args
            assert (counts == -7).all() and pb.stats() == stats
        assert lib.mbavo_pairs_prepare_points(None, sp, bp, ip(off), xp, zp, None) == E_ARG
        # NULL arrays with an empty total are fine
        assert lib.mbavo_pairs_prepare_points(pb.handle, sp, bp, ip([0, 0, 0, 0]), None, None, None) == 0
        assert [pb.array[e].K for e in range(B * L)] == [0] * (B * L)
        again = pb.prepare_points(sharp, blur, points)
        assert np.array_equal(again, good)
        dv.assert_twins(dv.read_batch(pb, again), held, "after the errors")
        # a list exactly at the capacity passes
        assert lib.mbavo_pairs_prepare_points(pb.handle, sp, bp, ip([0, 0, 0, cap]), _t(np.zeros((cap, 2))).data_ptr(), _t(np.ones(cap)).data_ptr(), None) == 0
        ustats = pb.step_stats()[0]
        for args, want in (((bp, 1, ip([1]), None, ip([0, 5]), xp, zp), E_ARG), ((bp, 1, None, sp, ip([0, 5]), xp, zp), E_ARG),
                           ((bp, 1, ip([1]), sp, None, xp, zp), E_ARG), ((bp, 1, ip([1]), sp, ip([0, 5]), None, zp), E_ARG),
                           ((bp, 1, ip([3]), sp, ip([0, 5]), xp, zp), E_ARG), ((bp, 2, ip([1, 1]), sp, ip([0, 2, 5]), xp, zp), E_ARG),
                           ((bp, 2, ip([0, 1]), sp, ip([0, 5, 2]), xp, zp), E_ARG), ((bp, 1, ip([1]), sp, ip([2, 5]), xp, zp), E_ARG),
                           ((bp, -1, ip([1]), sp, ip([0, 5]), xp, zp), E_ARG), ((bp, 1, ip([1]), sp, ip([0, cap + 1]), xp, zp), E_RANGE)):
            assert lib.mbavo_pairs_update_points(pb.handle, *args, None) == want, args
            assert pb.step_stats()[0] == ustats
        assert pb.update_points(blur, [1], sharp[:1].contiguous(), [c["lists"][5]])[1, 0] > 0
        # an object with a raw camera before its camera call
        raw = dv.dev(cases.valid_case()["sharp"], cases.valid_case()["blur"])
        off5 = ip([0, 5, 5, 5])
        assert lib.mbavo_pairs_prepare_points(cam.handle, raw[0].data_ptr(), raw[1].data_ptr(), off5, xp, zp, None) == E_ARG
        assert cam.stats()[:3] == (0, 0, 0)
        assert cam.set_camera(cases.valid_camera("radtan")) == 0
        assert lib.mbavo_pairs_prepare_points(cam.handle, raw[0].data_ptr(), raw[1].data_ptr(), off5, xp, zp, None) == 0
    finally:
        pb.close()
        cam.close()


# ---- check 6: the launch witness
@pytest.mark.parametrize("dense", [True, False])
def test_launches_do_not_depend_on_B(mbavo, gpu_ctx, dense):
    """prepare_points: ceil((L-1)/3) + 2 launches, one synchronisation, 4 B L bytes back; update_points with keyframes: one copy
    kernel more; the detector route needs one launch more with a grid and two more with every candidate; the device bytes are the
    plan's."""
    seen = []
    for n in (3, 40):
        sharp, blur = dv.dev(_images(n, H, W, 1), _images(n, H, W, 2))
        points = [_list(5 + (b % 7), H, W, BORDERS, b) for b in range(n)]
        pb, det = _object(gpu_ctx, dense, pairs=n), _object(gpu_ctx, dense, pairs=n)
        try:
            pb.prepare_points(sharp, blur, points)
            det.prepare(sharp, _t(np.full((n, H, W), 1.5, np.float32)), blur)
            assert pb.stats() == (1 + 2, 1, 4 * n * L, _capacity(gpu_ctx, pb)[1])
            assert det.stats()[0] == pb.stats()[0] + (2 if dense else 1) and det.stats()[3] == pb.stats()[3]
            keys = [0, n - 1]
            pb.update_points(blur, keys, sharp[:2].contiguous(), points[:2])
            assert pb.step_stats()[0] == (1 + 1 + 2, 1, 4 * n * L)
            pb.update_points(blur, [], None, [])
            assert pb.step_stats()[0] == (1, 1, 0)
            seen.append((pb.stats()[:2], det.stats()[:2]))
        finally:
            pb.close()
            det.close()
    assert seen[0] == seen[1]


# ---- check 7: a frame through track_frame_points
def test_a_frame_through_track_frame_points_equals_the_four_calls(mbavo, gpu_ctx):
    capi, lib = mbavo.capi, gpu_ctx.lib
    n, levels, k = 2, 2, 2
    case = ps.assess_inputs(n, 120, 160, k)
    states = pt.make_states(capi, case)
    first = ps.host_keypoints0(case, 4)
    new_sharp = np.ascontiguousarray(np.roll(case["sharp"][1:2], (2, 3), (1, 2)))
    newer = [(np.ascontiguousarray(first[1][0][::2]), np.ascontiguousarray(first[1][1][::2]))]
    from mba_vo_amd import workloads
    make = lambda: workloads.PairBatch(gpu_ctx, n, L=levels, H=120, W=160, k=k, N=ps.N_KNOTS, cell=0, every_candidate=True, thresh=ps.THR, border=4)
    one, hand = make(), make()
    o = lms.lm_batch_opts(capi, k, 3)
    try:
        sharp, blur = dv.dev(case["sharp"], case["blur"])
        for pb in (one, hand):
            c0 = pb.prepare_points(sharp, blur, first)
            assert c0[:, 0].tolist() == [len(f[1]) for f in first] and (c0 > 0).all()
            assert pb.set_states(states) == 0
        frames, counts, res, _ = one.track_frame_points(blur, case["cap"], case["exp"], o, THRESHOLDS, [1], dv.dev(new_sharp)[0], newer)
        hcounts = hand.update_points(blur, [1], dv.dev(new_sharp)[0], newer)
        assert hand.predict(case["cap"], case["exp"]) == 0
        hres = (capi.LmBatchResult * n)()
        assert lib.mbavo_lm_batch_levels(gpu_ctx.handle, n, levels, hand.array, C.byref(o), hres, None, 0) == 0
        hframes = hand.commit(*THRESHOLDS)
        assert np.array_equal(counts, hcounts) and counts[1, 0] == len(newer[0][1]) and np.array_equal(counts[0], c0[0])
        assert one.step_stats()[0] == hand.step_stats()[0] and one.track_stats() == hand.track_stats()
        gk, hk = one.knots(), hand.knots()
        worst = max(float(np.abs(gk[0] - hk[0]).max()), float(np.abs(gk[1] - hk[1]).max()))
        print("track_frame_points against the four calls: max knot difference %.3e, same bits: %s" % (worst, bytes(frames) == bytes(hframes)))
        assert worst <= ps.KNOT_TOL
        for b in range(n):
            f, h_ = frames[b], hframes[b]
            assert f.a.status == h_.a.status == 0 and f.a.is_keyframe == h_.a.is_keyframe and f.a.num_keypoints0 == h_.a.num_keypoints0 == counts[b, 0]
            assert np.abs(np.array(f.T_world) - np.array(h_.T_world)).max() <= ps.KNOT_TOL
            assert (res[b].iterations, res[b].num_outliers) == (hres[b].iterations, hres[b].num_outliers)
        # the error rules of mbavo_pairs_track_frame: a NULL among h_cap, h_exp, opts, h_out, nothing launched
        before = one.step_stats()[0], one.track_stats()
        off = capi.ip(np.array([0, 0], np.int32))
        args = [one.handle, blur.data_ptr(), 0, None, None, off, None, None, capi.dp(case["cap"]), capi.dp(case["exp"]), C.byref(o), None, None, 0,
                THRESHOLDS[0], THRESHOLDS[1], THRESHOLDS[2], (capi.PairsFrame * n)(), None]
        for hole in (8, 9, 10, 17):
            a = list(args)
            a[hole] = None
            assert lib.mbavo_pairs_track_frame_points(*a) == E_ARG, hole
        assert (one.step_stats()[0], one.track_stats()) == before
    finally:
        one.close()
        hand.close()
