"""A set of G cameras in one batch of pairs on the device (mbavo_pairs_opts.num_cameras, mbavo_pairs_set_cameras) and the batched
map (mbavo_undistort_map_batch).

The batched map is held bit for bit to the single calls and to numpy (tests/pairs_cameras_ref.py).  The object is held to what
exists: a B = 4, G = 3 object against four objects of ONE pair each, built the old way (num_cameras = 0, the pair's own
`intrinsics`, mbavo_pairs_set_camera / _unified) and fed the pair's slice of the inputs -- every array, every problem's intrinsics,
the assessments, the LM's records and the tracked frames, after a prepare, after updates and after a second set_cameras.

Shapes: 48 x 64 from a 52 x 76 raw camera, L = 3 (the last odd pixel pair, image starts off a word, a third level), and 45 x 63
(an odd pixel count: camera 1's map starts off a 16-byte boundary and the remap's byte branch runs).  Pairs 0 and 2 share camera
0, the index pattern (0, 1, 0, 2) does not ascend.  Every test asserts the witnesses of the set (_witness)."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_cameras_ref as cref
import pairs_cases as cases
import pairs_device as dv
import pairs_step as ps
import pairs_undistort_ref as uref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
B, G, L = 4, 3, 3
CELL, THR, BORDERS = cases.CELL, cases.THR, cases.BORDERS
DEPTH_FORMATS = cases.DEPTH_FORMATS
IDX = list(cref.CAMERA_OF_PAIR)

_CASES = {}


def _case(geometry):
    """Everything numpy of one geometry, made once and left unchanged: the cameras and their maps, three sets of images (raw
    Hs x Ws for undistort != 0 and pinhole H x W for undistort = 0) and depth maps in both geometries and the three formats."""
    if geometry not in _CASES:
        H, W, Hs, Ws = cref.GEOMETRIES[geometry]
        cams = cref.cameras(geometry)
        tex = lambda h, w, seed: np.stack([synth.texture_image(h, w, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        seeds = dict(sharp=7, blur=107, new_sharp=40, new_blur=140, blur3=171)
        _CASES[geometry] = dict(
            geometry=geometry, H=H, W=W, Hs=Hs, Ws=Ws, cams=cams, maps=cref.maps_of(cams, H, W),
            raw={k: tex(Hs, Ws, s) for k, s in seeds.items()}, pin={k: tex(H, W, s) for k, s in seeds.items()},
            depth={(und2, fmt, k): cases.raw_depth(fmt, B, Hs if und2 else H, Ws if und2 else W, seed=31 + fmt + (50 if k == "new" else 0) + (7 if und2 else 0))
                   for und2 in (False, True) for fmt in (0, 1, 2) for k in ("old", "new")})
    return _CASES[geometry]


def _witness(c):
    """What the set is there for: camera 0's taps outside the raw image, three to_intrinsics that differ in every entry."""
    share = float(uref.tap_outside(c["maps"][0], c["Hs"], c["Ws"]).mean())
    assert 0.01 < share < 0.10, share
    K = [cam["to_intr"] for cam in c["cams"]]
    assert all(K[i][a] != K[j][a] for i in range(G) for j in range(i + 1, G) for a in range(4))
    assert IDX == [0, 1, 0, 2]
    return share


def _single_camera(cam):
    from mba_vo_amd import workloads
    if cam["model"] == 2:
        return workloads.camera_unified(cam["Hs"], cam["Ws"], cam["from_intr"], cam["xi"], cam["dist"])
    return workloads.camera_radtan(cam["Hs"], cam["Ws"], cam["from_intr"], cam["dist"])


def _set_camera(cam):
    from mba_vo_amd import workloads
    return workloads.pairs_camera(_single_camera(cam), cam["to_intr"])


def _set_of(c):
    return [_set_camera(cam) for cam in c["cams"]]


def _object(ctx, c, undistort, dense, fmt=0, pairs=B, num_cameras=G, intr=None, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, pairs, L=L, H=c["H"], W=c["W"], intr=intr, border=list(BORDERS), cell=0 if dense else CELL, thresh=THR,
                               every_candidate=dense, undistort=undistort, num_cameras=num_cameras, **dict(DEPTH_FORMATS[fmt], **kw))


def _single(ctx, c, g, undistort, dense, fmt=0, **kw):
    """An object of ONE pair that looks through camera g, built without the feature."""
    cam = c["cams"][g]
    pb = _object(ctx, c, undistort, dense, fmt, pairs=1, num_cameras=0, intr=cam["to_intr"], **kw)
    if undistort:
        assert pb.set_camera(_single_camera(cam)) == 0
    return pb


def _inputs(c, undistort, fmt, which="old"):
    """(sharp, depth, blur) numpy of all B pairs for an object of that kind: `old` the first set, `new` the second."""
    img = c["raw"] if undistort else c["pin"]
    depth = c["depth"][(undistort == 2, fmt, which)]
    return (img["sharp"], depth, img["blur"]) if which == "old" else (img["new_sharp"], depth, img["new_blur"])


def _rows(a, rows):
    return np.ascontiguousarray(a[list(rows)])


def _assert_equals_singles(multi, counts, singles, single_counts, tag):
    """Every array of the B-pair object, pair by pair, against the one-pair objects; and every problem's intrinsics."""
    got = dv.read_batch(multi, counts)
    for b, (pb, cb) in enumerate(zip(singles, single_counts)):
        assert np.array_equal(counts[b], cb[0]), (tag, b, counts[b], cb)
        dv.assert_twins(got[b * L:(b + 1) * L], dv.read_batch(pb, cb), (tag, b))
        for l in range(L):
            assert list(multi.array[b * L + l].intrinsics) == list(pb.array[l].intrinsics), (tag, b, l)
    return got


def _close(*objs):
    for o in objs:
        for pb in (o if isinstance(o, (list, tuple)) else [o]):
            pb.close()


# ---- check 1: the batched map
@pytest.mark.parametrize("geometry", ["crop", "odd"])
def test_map_batch_equals_the_single_calls_and_numpy(mbavo, gpu_ctx, geometry):
    """Every entry of all three maps in one launch: the bits of mbavo_undistort_map / _map_unified per camera and of numpy; n = 1;
    and into a buffer that is only 8-byte aligned, its neighbours untouched."""
    import torch
    from mba_vo_amd import workloads
    c = _case(geometry)
    _witness(c)
    H, W = c["H"], c["W"]
    cams = _set_of(c)
    got = workloads.undistort_map_batch(gpu_ctx, cams, H, W).cpu().numpy()
    assert got.dtype == np.float32 and dv.same_bits(got, c["maps"])
    for g, cam in enumerate(c["cams"]):
        one = workloads.undistort_map(gpu_ctx, _single_camera(cam), cam["to_intr"], H, W).cpu().numpy()
        assert dv.same_bits(got[g], one), g
        assert dv.same_bits(workloads.undistort_map_batch(gpu_ctx, [cams[g]], H, W).cpu().numpy()[0], one), g
    buf = torch.full((G * 2 * H * W + 4,), -7.0, dtype=torch.float32, device="cuda:0")
    arr = (mbavo.capi.PairsCamera * G)(*cams)
    assert gpu_ctx.lib.mbavo_undistort_map_batch(gpu_ctx.handle, G, arr, H, W, buf.data_ptr() + 8) == 0
    out = buf.cpu().numpy()
    assert dv.same_bits(out[2:-2].reshape(G, H, W, 2), c["maps"]) and np.all(out[:2] == -7.0) and np.all(out[-2:] == -7.0)


def test_map_batch_rejects_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    import torch
    c = _case("crop")
    H, W = c["H"], c["W"]
    lib, capi = gpu_ctx.lib, mbavo.capi
    out = torch.full((G, H, W, 2), -7.0, dtype=torch.float32, device="cuda:0")
    o = out.data_ptr()

    def cams(**kw):
        s = _set_of(c)
        k = s[kw.get("at", 1)]
        for name in ("model", "H", "W", "xi"):
            if name in kw:
                setattr(k, name, kw[name])
        for i in kw.get("zero", ()):
            k.intrinsics[i] = 0.0
        for i in kw.get("zero_to", ()):
            k.to_intrinsics[i] = 0.0
        return (capi.PairsCamera * G)(*s)

    good = cams()
    for args in ((G, None, H, W, o), (G, good, H, W, None), (0, good, H, W, o), (-1, good, H, W, o), (65536, good, H, W, o), (G, good, 0, W, o),
                 (G, good, H, -1, o), (G, good, 2048, 2049, o), (G, cams(model=0), H, W, o), (G, cams(model=3), H, W, o), (G, cams(H=0), H, W, o),
                 (G, cams(at=0, W=0), H, W, o), (G, cams(H=4096, W=1025), H, W, o), (G, cams(zero=(0,)), H, W, o), (G, cams(at=2, zero=(1,)), H, W, o),
                 (G, cams(zero_to=(0,)), H, W, o), (G, cams(at=0, zero_to=(1,)), H, W, o), (G, cams(xi=-1.0), H, W, o), (G, cams(xi=float("nan")), H, W, o)):
        assert lib.mbavo_undistort_map_batch(gpu_ctx.handle, *args) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.mbavo_undistort_map_batch(gpu_ctx.handle, G, cams(at=0, xi=-1.0), H, W, o) == 0  # (model 1 does not read xi) and good arguments write
    torch.cuda.synchronize()
    assert dv.same_bits(out.cpu().numpy(), c["maps"])


# ---- check 2: the object after a prepare
@pytest.mark.parametrize("undistort", [0, 1, 2])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_prepare_equals_one_pair_objects(mbavo, gpu_ctx, undistort, fmt, dense):
    """B = 4, G = 3 against four num_cameras = 0 objects of one pair: pyramid levels, gradient images, keypoints, depths, counts and
    the problems' intrinsics, bit for bit; with raw images level 0 is numpy's remap through the camera's map.  Format 1 is where
    the pair's own ray divides the depth."""
    c = _case("crop")
    _witness(c)
    sharp, depth, blur = _inputs(c, undistort, fmt)
    multi = _object(gpu_ctx, c, undistort, dense, fmt)
    singles = [_single(gpu_ctx, c, g, undistort, dense, fmt) for g in IDX]
    try:
        assert multi.set_cameras(_set_of(c), IDX) == 0
        counts = multi.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0])
        cs = [pb.prepare(dv.dev(_rows(sharp, [b]))[0], dv.dev_depth(_rows(depth, [b])), dv.dev(_rows(blur, [b]))[0]) for b, pb in enumerate(singles)]
        assert counts.min() > 0
        got = _assert_equals_singles(multi, counts, singles, cs, (undistort, fmt, dense))
        K = cref.level_intrinsics(c["cams"], IDX, L)
        for e in range(B * L):
            assert list(multi.array[e].intrinsics) == K[e // L, e % L].tolist()
        if undistort:
            und_s, und_b = cref.remapped(sharp, c["maps"], IDX), cref.remapped(blur, c["maps"], IDX)
            for b in range(B):
                assert np.array_equal(got[b * L]["ref"], und_s[b].ravel()) and np.array_equal(got[b * L]["cur"], und_b[b].ravel())
        if fmt == 1:  # the ray matters: pairs 0 and 3 given each other's camera would keep other depths
            assert not np.array_equal(K[0, 0], K[3, 0])
    finally:
        _close(multi, singles)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("kf", [0, 2])
def test_prepare_on_an_odd_pixel_count(mbavo, gpu_ctx, dense, kf):
    """45 x 63: map g starts at byte 8 * 2835 * g, camera 1's off a 16-byte boundary, and an image is 2835 bytes: the byte branch
    of the remap.  The same comparison, also with packed keyframes."""
    c = _case("odd")
    _witness(c)
    assert (8 * c["H"] * c["W"]) % 16 == 8
    sharp, depth, blur = _inputs(c, 1, 0)
    multi = _object(gpu_ctx, c, 1, dense, keyframe_format=kf)
    singles = [_single(gpu_ctx, c, g, 1, dense, keyframe_format=kf) for g in IDX]
    try:
        assert multi.set_cameras(_set_of(c), IDX) == 0
        counts = multi.prepare(*dv.dev(sharp, depth, blur))
        cs = [pb.prepare(*dv.dev(_rows(sharp, [b]), _rows(depth, [b]), _rows(blur, [b]))) for b, pb in enumerate(singles)]
        got = _assert_equals_singles(multi, counts, singles, cs, ("odd", dense, kf))
        und = cref.remapped(sharp, c["maps"], IDX)
        for b in range(B):
            assert np.array_equal(got[b * L]["ref"], und[b].ravel())
    finally:
        _close(multi, singles)


@pytest.mark.parametrize("geometry", ["crop", "odd"])
def test_both_images_from_one_map_read_write_the_same_bytes(mbavo, gpu_ctx, geometry, monkeypatch):
    """A prepare of a camera-set object remaps both images of a pair in one lane, from one read of the map entries; with
    MBAVO_PAIRS_REMAP_BOTH=0 (an override of the environment layer, read at creation) it remaps them in two grid rows as an update does.  The same bytes in every
    array, the same launches; 45 x 63 takes the byte path in both."""
    c = _case(geometry)
    _witness(c)
    sharp, depth, blur = _inputs(c, 1, 0)
    both = _object(gpu_ctx, c, 1, False)
    monkeypatch.setenv("MBAVO_PAIRS_REMAP_BOTH", "0")
    gpu_ctx.lib.mbavo_reload_env()
    try:
        rows = _object(gpu_ctx, c, 1, False)
    finally:
        monkeypatch.delenv("MBAVO_PAIRS_REMAP_BOTH")
        gpu_ctx.lib.mbavo_reload_env()
    try:
        for pb in (both, rows):
            assert pb.set_cameras(_set_of(c), IDX) == 0
        cb, cr = both.prepare(*dv.dev(sharp, depth, blur)), rows.prepare(*dv.dev(sharp, depth, blur))
        assert np.array_equal(cb, cr) and both.stats() == rows.stats()
        got = dv.read_batch(both, cb)
        dv.assert_twins(got, dv.read_batch(rows, cr), ("both", geometry))
        und_s, und_b = cref.remapped(sharp, c["maps"], IDX), cref.remapped(blur, c["maps"], IDX)
        for b in range(B):
            assert np.array_equal(got[b * L]["ref"], und_s[b].ravel()) and np.array_equal(got[b * L]["cur"], und_b[b].ravel())
    finally:
        _close(both, rows)


# ---- check 3: updates
@pytest.mark.parametrize("undistort", [0, 1, 2])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_updates_equal_one_pair_objects(mbavo, gpu_ctx, undistort, fmt, dense):
    """After an update with n_key = 2 that lists pairs 1 and 3 and brings new blurred frames for all pairs; after an update with
    n_key = 0; and after a second set_cameras that exchanges the cameras of pairs 1 and 3 followed by an update that lists
    exactly those pairs (their one-pair objects are made anew with the other camera and prepared on the same images)."""
    c = _case("crop")
    _witness(c)
    sharp, depth, blur = _inputs(c, undistort, fmt)
    new_sharp, new_depth, new_blur = _inputs(c, undistort, fmt, "new")
    blur3 = (c["raw"] if undistort else c["pin"])["blur3"]
    keys = [1, 3]
    multi = _object(gpu_ctx, c, undistort, dense, fmt)
    singles = [_single(gpu_ctx, c, g, undistort, dense, fmt) for g in IDX]
    one = lambda a, b: (dv.dev_depth if a.dtype != np.uint8 else lambda x: dv.dev(x)[0])(_rows(a, [b]))
    try:
        assert multi.set_cameras(_set_of(c), IDX) == 0
        before = multi.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0])
        for b, pb in enumerate(singles):
            pb.prepare(one(sharp, b), one(depth, b), one(blur, b))
        # new keyframes for pairs 1 and 3, new blurred frames for all
        counts = multi.update(dv.dev(new_blur)[0], keys, dv.dev(_rows(new_sharp, keys))[0], dv.dev_depth(_rows(new_depth, keys)))
        cs = [pb.update(one(new_blur, b), [0], one(new_sharp, b), one(new_depth, b)) if b in keys else pb.update(one(new_blur, b))
              for b, pb in enumerate(singles)]
        assert np.array_equal(counts[0], before[0]) and not np.array_equal(counts[keys], before[keys])
        _assert_equals_singles(multi, counts, singles, cs, ("keys", undistort, fmt, dense))
        # n_key == 0
        counts = multi.update(dv.dev(blur3)[0])
        cs = [pb.update(one(blur3, b)) for b, pb in enumerate(singles)]
        _assert_equals_singles(multi, counts, singles, cs, ("blur only", undistort, fmt, dense))
        # the cameras of pairs 1 and 3 exchanged; exactly those pairs get a new keyframe
        swapped = list(cref.SWAPPED)
        assert multi.set_cameras(_set_of(c), swapped) == 0
        counts = multi.update(dv.dev(blur)[0], keys, dv.dev(_rows(sharp, keys))[0], dv.dev_depth(_rows(depth, keys)))
        cs = []
        for b in range(B):
            if b in keys:
                singles[b].close()
                singles[b] = _single(gpu_ctx, c, swapped[b], undistort, dense, fmt)
                cs.append(singles[b].prepare(one(sharp, b), one(depth, b), one(blur, b)))
            else:
                cs.append(singles[b].update(one(blur, b)))
        _assert_equals_singles(multi, counts, singles, cs, ("swapped", undistort, fmt, dense))
        K = cref.level_intrinsics(c["cams"], swapped, L)
        assert list(multi.array[1 * L].intrinsics) == K[1, 0].tolist() == list(c["cams"][2]["to_intr"])
    finally:
        _close(multi, singles)


def _motion():
    m = ps.assess_inputs(B, 48, 64, 4)
    return m["cap"], m["exp"], m["t0"], m["dt"], m["kt"], m["kR"]


def _prepared_with_motion(ctx, c, undistort, fmt, dense):
    """The B-pair object and the one-pair objects, prepared and given the same knots (N = 6, degree 4)."""
    cap, exp, t0, dt, kt, kR = _motion()
    sharp, depth, blur = _inputs(c, undistort, fmt)
    kw = dict(N=ps.N_KNOTS, k=4, S=2, pattern=np.array([[0, 0]], np.int32))
    multi = _object(ctx, c, undistort, dense, fmt, **kw)
    singles = [_single(ctx, c, g, undistort, dense, fmt, **kw) for g in IDX]
    assert multi.set_cameras(_set_of(c), IDX) == 0
    counts = multi.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0])
    assert counts.min() > 0
    assert multi.set_motion(cap, exp, t0, dt, kt, kR) == 0
    for b, pb in enumerate(singles):
        cb = pb.prepare(dv.dev(_rows(sharp, [b]))[0], dv.dev_depth(_rows(depth, [b])), dv.dev(_rows(blur, [b]))[0])
        assert np.array_equal(cb[0], counts[b])
        assert pb.set_motion(cap[b:b + 1], exp[b:b + 1], t0[b:b + 1], dt, kt[b:b + 1], kR[b:b + 1]) == 0
    return multi, singles


# ---- check 4: the assessment
@pytest.mark.parametrize("undistort,fmt", [(0, 0), (1, 1), (2, 1)])
def test_assessments_equal_one_pair_objects(mbavo, gpu_ctx, undistort, fmt):
    """mbavo_pairs_assess with every pair's own intrinsics: every field of every pair, bit for bit, what its one-pair object
    returns under the same knots (the sums are reduced in a fixed order for any B).  With another camera's intrinsics the
    averages are others: pair 3's, recomputed by a one-pair object that looks through camera 0, differ."""
    c = _case("crop")
    _witness(c)
    multi, singles = _prepared_with_motion(gpu_ctx, c, undistort, fmt, False)
    try:
        got = multi.assess(ps.FLOW0, ps.FLOW1, ps.KERNEL)
        want = [pb.assess(ps.FLOW0, ps.FLOW1, ps.KERNEL)[0] for pb in singles]
        for b in range(B):
            assert bytes(got[b]) == bytes(want[b]), (b, got[b].avg_flow, want[b].avg_flow)
            assert got[b].status == 0 and got[b].num_keypoints0 > 0 and got[b].avg_flow > 0
        assert multi.step_stats()[1] == (1, 1, C.sizeof(mbavo.capi.PairsAssessment) * B)  # one launch, one copy, one synchronisation
        if undistort == 0:  # (the same images and keypoints under camera 0's intrinsics: the test would see a shared K)
            cap, exp, t0, dt, kt, kR = _motion()
            sharp, depth, blur = _inputs(c, 0, fmt)
            other = _single(gpu_ctx, c, 0, 0, False, fmt, N=ps.N_KNOTS, k=4, S=2, pattern=np.array([[0, 0]], np.int32))
            try:
                other.prepare(dv.dev(_rows(sharp, [3]))[0], dv.dev_depth(_rows(depth, [3])), dv.dev(_rows(blur, [3]))[0])
                assert other.set_motion(cap[3:], exp[3:], t0[3:], dt, kt[3:], kR[3:]) == 0
                assert bytes(other.assess(ps.FLOW0, ps.FLOW1, ps.KERNEL)[0]) != bytes(got[3])
            finally:
                other.close()
    finally:
        _close(multi, singles)


# ---- check 5: the LM
@pytest.mark.parametrize("undistort,fmt", [(0, 0), (1, 1)])
def test_lm_on_the_object_equals_lm_on_the_one_pair_objects(mbavo, gpu_ctx, undistort, fmt):
    """mbavo_lm_batch_levels on the object's own array against the same call on an array of the same B x L shape assembled from
    the one-pair objects' problems: results, trace records and final knots.  The arrays the LM reads are identical and the layout
    is the same, so the expectation is equality of bits."""
    capi = mbavo.capi
    c = _case("crop")
    _witness(c)
    multi, singles = _prepared_with_motion(gpu_ctx, c, undistort, fmt, False)
    try:
        arr = (capi.Problem * (B * L))()
        for b, pb in enumerate(singles):
            for l in range(L):
                C.memmove(C.byref(arr, (b * L + l) * C.sizeof(capi.Problem)), C.byref(pb.array[l]), C.sizeof(capi.Problem))
        for e in range(B * L):
            assert arr[e].K == multi.array[e].K and list(arr[e].intrinsics) == list(multi.array[e].intrinsics)
        f_m, r_m, kinds = dv.run_lm(gpu_ctx, capi, B, L, multi.array, 4)
        f_s, r_s, _ = dv.run_lm(gpu_ctx, capi, B, L, arr, 4)
        kt, kR = multi.knots()
        same = f_m == f_s and r_m == r_s
        for b, pb in enumerate(singles):
            st, sR = pb.knots()
            print("pair %d: records equal %s, max |knot difference| %.3e" % (b, f_m[b] == f_s[b] and r_m[b] == r_s[b],
                                                                            max(np.abs(kt[b] - st[0]).max(), np.abs(kR[b] - sR[0]).max())))
            same = same and dv.same_bits(kt[b], st[0]) and dv.same_bits(kR[b], sR[0])
        assert sum(len(r) for r in r_m) > 0 and same
    finally:
        _close(multi, singles)


# ---- check 6: tracked frames
def _track(capi, pb, n, blur_t, keys, sharp_t, depth_t, cap):
    out, counts, res, trace = pb.track_frame(blur_t, np.full(n, cap), np.full(n, 0.02), lms.lm_batch_opts(capi, 2, 3), (ps.FLOW0, ps.FLOW1, ps.KERNEL),
                                             keys, sharp_t, depth_t, trace_cap=16)
    recs = [bytes(trace[b * 16 + i]) for b in range(n) for i in range(min(res[b].num_trace, 16))]
    return [bytes(out[b]) for b in range(n)], counts, [bytes(res[b]) for b in range(n)], recs


@pytest.mark.parametrize("undistort,fmt", [(1, 1), (0, 0)])
def test_track_frame_equals_one_pair_objects(mbavo, gpu_ctx, undistort, fmt):
    """mbavo_pairs_track_frame over two frames, the second with a new keyframe for pair 2: the mbavo_pairs_frame bytes (the
    assessment and T_world), the LM results and the states afterwards against the one-pair objects, expected identical (the
    arrays the LM reads and its layout per pair are the same)."""
    capi = mbavo.capi
    c = _case("crop")
    _witness(c)
    sharp, depth, blur = _inputs(c, undistort, fmt)
    new_sharp, new_depth, new_blur = _inputs(c, undistort, fmt, "new")
    blur3 = (c["raw"] if undistort else c["pin"])["blur3"]
    kw = dict(S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
    multi = _object(gpu_ctx, c, undistort, False, fmt, **kw)
    singles = [_single(gpu_ctx, c, g, undistort, False, fmt, **kw) for g in IDX]
    one = lambda a, b: (dv.dev_depth if a.dtype != np.uint8 else lambda x: dv.dev(x)[0])(_rows(a, [b]))
    try:
        assert multi.set_cameras(_set_of(c), IDX) == 0
        multi.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0])
        assert multi.set_states(multi.initial_states(0.0, 0.1)) == 0
        f1 = _track(capi, multi, B, dv.dev(new_blur)[0], [], None, None, 0.1)
        f2 = _track(capi, multi, B, dv.dev(blur3)[0], [2], one(new_sharp, 2), one(new_depth, 2), 0.2)
        states = multi.get_states()
        for b, pb in enumerate(singles):
            pb.prepare(one(sharp, b), one(depth, b), one(blur, b))
            assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
            g1 = _track(capi, pb, 1, one(new_blur, b), [], None, None, 0.1)
            g2 = _track(capi, pb, 1, one(blur3, b), [0] if b == 2 else [], one(new_sharp, b) if b == 2 else None, one(new_depth, b) if b == 2 else None, 0.2)
            for f, g, tag in ((f1, g1, "first"), (f2, g2, "second")):
                assert np.array_equal(f[1][b], g[1][0]), (tag, b)
                fr, gr = capi.PairsFrame.from_buffer_copy(f[0][b]), capi.PairsFrame.from_buffer_copy(g[0][0])
                print("%s frame, pair %d: max |T_world difference| %.3e" % (tag, b, np.abs(np.array(fr.T_world) - np.array(gr.T_world)).max()))
                assert fr.a.status == 0 and f[0][b] == g[0][0] and f[2][b] == g[2][0], (tag, b)
            assert bytes(states[b]) == bytes(pb.get_states()[0]), b
        assert len(f1[3]) > 0 and multi.track_stats() == ((1, 0, 0), (1, 1, C.sizeof(capi.PairsFrame) * B))
    finally:
        _close(multi, singles)


# ---- check 7: launches, synchronisations, bytes
@pytest.mark.parametrize("undistort", [0, 1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_stats_are_those_of_an_object_with_one_camera(mbavo, gpu_ctx, undistort, dense):
    """mbavo_pairs_last_stats, _update_stats and _track_stats of the G-camera object equal those of a num_cameras = 0 object of
    the same shape, call by call; the device bytes differ by the G - 1 further maps (by nothing with undistort = 0).  set_cameras
    belongs to none of them and the counters stay where they were.  What this test cannot show is set_cameras' own cost -- one
    launch (none with undistort = 0) and no synchronisation: the library has no counter for that call, so that statement rests on
    the code (PairBatch::set_cameras: one copy, one launch, no stream synchronisation) and on the timing of
    tools/pairs_cameras_bench.py."""
    capi = mbavo.capi
    c = _case("crop")
    _witness(c)
    sharp, depth, blur = _inputs(c, undistort, 0)
    new_sharp, new_depth, new_blur = _inputs(c, undistort, 0, "new")
    keys = [1, 3]
    kw = dict(S=2, k=2, N=2, pattern=np.array([[0, 0]], np.int32))
    multi = _object(gpu_ctx, c, undistort, dense, **kw)
    plain = _object(gpu_ctx, c, undistort, dense, num_cameras=0, intr=c["cams"][0]["to_intr"], **kw)
    try:
        assert multi.stats()[:3] == (0, 0, 0)
        assert multi.set_cameras(_set_of(c), IDX) == 0
        assert multi.stats()[:3] == (0, 0, 0) and multi.step_stats() == ((0, 0, 0), (0, 0, 0)) and multi.track_stats() == ((0, 0, 0), (0, 0, 0))
        if undistort:
            assert plain.set_camera(_single_camera(c["cams"][0])) == 0
        aligned = lambda v: (v + 255) // 256 * 256
        extra = aligned(8 * c["H"] * c["W"] * G) - aligned(8 * c["H"] * c["W"]) if undistort else 0
        for pb in (multi, plain):
            pb.prepare(dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0])
        pyr, kp = 1, (3 if dense else 2)
        assert multi.stats()[:3] == plain.stats()[:3] == (pyr + 1 + kp + (1 if undistort else 0), 1, 4 * B * L)
        assert multi.stats()[3] - plain.stats()[3] == extra
        for pb in (multi, plain):
            pb.update(dv.dev(new_blur)[0], keys, dv.dev(_rows(new_sharp, keys))[0], dv.dev_depth(_rows(new_depth, keys)))
        assert multi.step_stats()[0] == plain.step_stats()[0] == (1 + pyr + 1 + kp, 1, 4 * B * L)
        for pb in (multi, plain):
            pb.update(dv.dev(blur)[0])
        assert multi.step_stats()[0] == plain.step_stats()[0] == (pyr + (1 if undistort else 0), 1, 0)
        assert multi.set_cameras(_set_of(c), list(cref.SWAPPED)) == 0  # (again: nothing counted, nothing waited for)
        assert multi.step_stats()[0] == (pyr + (1 if undistort else 0), 1, 0)
        for pb in (multi, plain):
            assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
            _track(capi, pb, B, dv.dev(new_blur)[0], keys, dv.dev(_rows(sharp, keys))[0], dv.dev_depth(_rows(depth, keys)), 0.1)
        assert multi.step_stats()[0] == plain.step_stats()[0] and multi.track_stats() == plain.track_stats() == ((1, 0, 0), (1, 1, C.sizeof(capi.PairsFrame) * B))
    finally:
        _close(multi, plain)


# ---- check 8: rejections
@pytest.mark.parametrize("undistort", [0, 1])
def test_rejections_change_nothing(mbavo, gpu_ctx, undistort):
    """Every rejection of include/mbavo.h: MBAVO_E_ARG, and the cameras before the call stay in force -- a prepare afterwards
    writes the bits of the prepare before, the problems keep their intrinsics.  Before the first set_cameras prepare, update
    and track_frame return MBAVO_E_ARG (with undistort = 0 as well); an object with a camera set refuses set_camera and
    set_camera_unified, an object without one refuses set_cameras."""
    from mba_vo_amd import workloads
    capi, lib = mbavo.capi, gpu_ctx.lib
    c = _case("crop")
    _witness(c)
    sharp, depth, blur = _inputs(c, undistort, 1)
    ts, td, tb = dv.dev(sharp)[0], dv.dev_depth(depth), dv.dev(blur)[0]
    multi = _object(gpu_ctx, c, undistort, False, 1)
    plain = _object(gpu_ctx, c, undistort, False, 1, num_cameras=0, intr=c["cams"][0]["to_intr"])
    try:
        # no cameras yet: nothing runs
        frames, t = (capi.PairsFrame * B)(), np.full(B, 0.1)
        assert lib.mbavo_pairs_prepare(multi.handle, ts.data_ptr(), td.data_ptr(), tb.data_ptr(), None) == E_ARG
        assert lib.mbavo_pairs_update(multi.handle, tb.data_ptr(), 0, None, None, None, None) == E_ARG
        assert lib.mbavo_pairs_track_frame(multi.handle, tb.data_ptr(), 0, None, None, None, capi.dp(t), capi.dp(t), C.byref(lms.lm_batch_opts(capi, 4, 3)),
                                           None, None, 0, ps.FLOW0, ps.FLOW1, ps.KERNEL, frames, None) == E_ARG
        assert multi.stats()[:3] == (0, 0, 0) and multi.step_stats()[0] == (0, 0, 0) and multi.track_stats() == ((0, 0, 0), (0, 0, 0))
        # the two kinds of object refuse each other's call
        assert multi.set_camera(_single_camera(c["cams"][0])) == E_ARG and multi.set_camera(_single_camera(c["cams"][1])) == E_ARG
        assert plain.set_cameras(_set_of(c), IDX) == E_ARG and plain.set_cameras(_set_of(c)[:1], [0] * B) == E_ARG
        assert lib.mbavo_pairs_prepare(multi.handle, ts.data_ptr(), td.data_ptr(), tb.data_ptr(), None) == E_ARG  # still none
        # the first cameras, and what a prepare writes under them
        assert multi.set_cameras(_set_of(c), IDX) == 0
        counts = multi.prepare(ts, td, tb)
        first = dv.read_batch(multi, counts)
        K = [list(multi.array[e].intrinsics) for e in range(B * L)]

        def cams(**kw):
            s = _set_of(c)
            for g in (range(G) if kw.get("all") else [kw.get("at", 1)]):
                for name in ("model", "H", "W", "xi"):
                    if name in kw:
                        setattr(s[g], name, kw[name])
            for i in kw.get("zero", ()):
                s[kw.get("at", 1)].intrinsics[i] = 0.0
            for i in kw.get("zero_to", ()):
                s[kw.get("at", 1)].to_intrinsics[i] = 0.0
            for i in range(4):  # (other cameras than the first call's wherever the call would go through)
                s[0].to_intrinsics[i] *= 1.01
            return s

        good = cams()
        arr = (capi.PairsCamera * G)(*good)
        idx = (C.c_int * B)(*cref.SWAPPED)
        assert lib.mbavo_pairs_set_cameras(multi.handle, G, None, idx) == E_ARG and lib.mbavo_pairs_set_cameras(multi.handle, G, arr, None) == E_ARG
        assert lib.mbavo_pairs_set_cameras(None, G, arr, idx) == E_ARG
        for s, i in ((good[:2], [0, 1, 0, 1]), (good + good[:1], list(cref.SWAPPED)), ([], list(cref.SWAPPED)),  # G != num_cameras
                     (good, [0, 1, 0, 3]), (good, [0, -1, 0, 2]), (good, [G, 1, 0, 2]),                        # an index outside 0 .. G-1
                     (cams(model=0), IDX), (cams(model=3), IDX), (cams(at=2, model=-1), IDX),                  # a model other than 1, 2
                     (cams(H=0), IDX), (cams(H=4096, W=1025, all=True), IDX), (cams(zero=(0,)), IDX), (cams(at=0, zero=(1,)), IDX),
                     (cams(xi=-0.5), IDX), (cams(xi=float("nan")), IDX), (cams(xi=float("inf")), IDX),      # what the single calls reject
                     (cams(H=c["Hs"] + 1), IDX), (cams(at=2, W=c["Ws"] - 1), IDX),                             # raw sizes that differ
                     (cams(zero_to=(0,)), IDX), (cams(at=2, zero_to=(1,)), IDX)):                              # fx or fy of to_intrinsics 0
            assert multi.set_cameras(s, i) == E_ARG, (len(s), i)
        assert [list(multi.array[e].intrinsics) for e in range(B * L)] == K
        again = multi.prepare(ts, td, tb)
        assert np.array_equal(again, counts)
        dv.assert_twins(dv.read_batch(multi, again), first, "after the rejections")
        # and the same cameras, accepted, do change what a prepare writes
        assert multi.set_cameras(good, list(cref.SWAPPED)) == 0
        assert [list(multi.array[e].intrinsics) for e in range(B * L)] != K
        if undistort:
            changed = dv.read_batch(multi, multi.prepare(ts, td, tb))
            assert not np.array_equal(changed[1 * L]["ref"], first[1 * L]["ref"])
    finally:
        _close(multi, plain)
