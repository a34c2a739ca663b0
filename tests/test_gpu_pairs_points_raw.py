"""The caller's points in the raw camera's geometry on the device (mbavo_undistort_points_batch,
mbavo_pairs_set_points_geometry), all through the C ABI.  The stand-alone entry is held bit for bit, NaNs by position, to the numpy
restatement of the header's inverse camera (tests/pairs_points_raw_ref.py, itself held to the round trip and to hand-made cases on
the CPU by tests/test_pairs_points_raw_api.py); the pairs batch to the restatement's composition with tests/pairs_points_ref.py,
to a second object fed the stand-alone entry's output in geometry 0, and in its launch statistics to a geometry-0 call.

Shapes: B = 3, L = 3, undistorted 64 x 48 from raw 80 x 60, undistort = 1, every_candidate = 1, a set of G = 2 cameras (one per
model, pairs -> cameras 0, 1, 0) or one camera; valid_radius 2 and 0.  The keypoint capacity of such an object is that of its
coarsest level, 16 x 12 = 192, and a longer row is MBAVO_E_RANGE, so the lists of these objects are 192 points long (one step of
the workgroup's 256-point loop); the 700-point lists that take three steps run on the same scene at twice the size (128 x 96 from
160 x 120, capacity 768).  An update lists its pairs in ascending order, as mbavo_pairs_update demands: [0, 2]."""
import ctypes as C

import numpy as np
import pytest

import pairs_api_support as api
import pairs_cameras_ref as cref
import pairs_device as dv
import pairs_points_raw_ref as rref
import pairs_undistort_ref as uref
import pairs_valid_ref as vref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
B, L = 3, 3
BORDERS = (3, 2, 1)
CAMERA_OF_PAIR = (0, 1, 0)
_CASES = {}


def _cams(scale):
    """The two cameras at scale 1 (64 x 48 from 80 x 60) or 2: the radial-tangential lens whose corners leave the raw image (and
    whose inverse has no solution out there), and a unified camera with xi = 1 and a mild distortion."""
    s = float(scale)
    H, W, Hs, Ws = 48 * scale, 64 * scale, 60 * scale, 80 * scale
    radtan = dict(model=1, Hs=Hs, Ws=Ws, from_intr=uref.intrinsics(Hs, Ws), xi=0.0, dist=uref.DIST_OUTSIDE,
                  to_intr=(38.0 * s, 37.5 * s, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2))
    unified = dict(model=2, Hs=Hs, Ws=Ws, from_intr=(110.0 * s, 109.0 * s, (Ws - 1) / 2 - 0.4, (Hs - 1) / 2 + 0.3), xi=1.0, dist=(3e-2, -4e-3, 2e-4, -1e-4),
                   to_intr=(33.0 * s, 32.5 * s, (W - 1) / 2 - 0.2, (H - 1) / 2 + 0.1))
    return [radtan, unified]


def _raw_list(cam, n, seed):
    """n raw points of a camera: the hand-made ones first, then random ones spread over and beyond the raw image -- whole, half and
    arbitrary coordinates -- with depths on both sides of 1e-2, every kept depth different (the order shows)."""
    rng = np.random.default_rng(seed)
    Hs, Ws = cam["Hs"], cam["Ws"]
    uv = np.stack([rng.uniform(-6, Ws + 5, n), rng.uniform(-6, Hs + 5, n)], 1)
    uv[::3] = np.floor(uv[::3])
    uv[1::6] = np.floor(uv[1::6]) + 0.5
    edge = np.array(rref.edge_points(cam))[:n]
    uv[:len(edge)] = edge
    z = 1.0 + 1e-3 * np.arange(n)
    z[rng.uniform(0, 1, n) < 0.08] = 0.005
    return np.ascontiguousarray(uv), np.ascontiguousarray(z)


def _case(scale):
    """Everything numpy of one size, made once and left unchanged."""
    if scale not in _CASES:
        cams = _cams(scale)
        H, W, Hs, Ws = 48 * scale, 64 * scale, 60 * scale, 80 * scale
        n = 192 if scale == 1 else 700
        tex = lambda seed, m=B: np.stack([synth.texture_image(Hs, Ws, seed=seed + 3 * b, octaves=(16, 8, 4)) for b in range(m)])
        maps = [cref.camera_map(c, H, W) for c in cams]
        valid0 = [vref.valid0(m, Hs, Ws) for m in maps]
        of_pair = [cams[g] for g in CAMERA_OF_PAIR]
        lists = [_raw_list(of_pair[0], n, 1), _raw_list(of_pair[1], n, 2), (np.zeros((0, 2)), np.zeros(0))]  # one of each model; pair 2: an empty list
        full = [_raw_list(of_pair[b], n, 10 + b) for b in range(B)]
        _CASES[scale] = dict(H=H, W=W, Hs=Hs, Ws=Ws, n=n, cams=cams, of_pair=of_pair, valid0=valid0, lists=lists, full=full,
                             sharp=tex(7), blur=tex(107), new_sharp=tex(40, 2), new_blur=tex(140))
    return _CASES[scale]


def _camera(cam):
    from mba_vo_amd import workloads
    if cam["model"] == 2:
        return workloads.camera_unified(cam["Hs"], cam["Ws"], cam["from_intr"], cam["xi"], cam["dist"])
    return workloads.camera_radtan(cam["Hs"], cam["Ws"], cam["from_intr"], cam["dist"])


def _pairs_cameras(cams):
    from mba_vo_amd import workloads
    return [workloads.pairs_camera(_camera(c), c["to_intr"]) for c in cams]


def _object(ctx, c, r, one=None, borders=BORDERS):
    """An every-candidate object of case c with valid_radius r: the set of two cameras, or (one = 0 / 1) that camera alone."""
    from mba_vo_amd import workloads
    kw = dict(L=L, H=c["H"], W=c["W"], border=list(borders), cell=0, thresh=3.0, every_candidate=True, undistort=1, valid_radius=r)
    if one is None:
        pb = workloads.PairBatch(ctx, B, num_cameras=2, **kw)
        assert pb.set_cameras(_pairs_cameras(c["cams"]), list(CAMERA_OF_PAIR)) == 0
    else:
        pb = workloads.PairBatch(ctx, B, intr=c["cams"][one]["to_intr"], **kw)
        assert pb.set_camera(_camera(c["cams"][one])) == 0
    return pb


def _clears(c, r, of_pair_index):
    if r == 0:
        return None
    return [vref.clearance(c["valid0"][g], L, r) for g in of_pair_index]


def _composed(ctx, cams_of_rows, lists):
    """The lists through mbavo_undistort_points_batch (row i through cams_of_rows[i]), then without the points outside the raw image
    (removed on the host): geometry-0 lists."""
    from mba_vo_amd import workloads
    import torch
    xy, ok, off = workloads.undistort_points_batch(ctx, _pairs_cameras(cams_of_rows), [q[0] for q in lists])
    torch.cuda.synchronize()
    xy = xy.cpu().numpy()
    out = []
    for i, ((uv, z), cam) in enumerate(zip(lists, cams_of_rows)):
        keep = rref.raw_inside(uv, cam["Hs"], cam["Ws"])
        out.append((np.ascontiguousarray(xy[off[i]:off[i + 1]][keep]), np.ascontiguousarray(z[keep])))
    return out


def _assert_keypoints(got, want, counts, want_counts, tag):
    assert np.array_equal(counts, want_counts), (tag, counts, want_counts)
    for e, (g, w) in enumerate(zip(got, want)):
        assert dv.same_bits(g["xy"], w["xy"]) and dv.same_bits(g["z"], w["z"]), (tag, e)


def _nan_equal_bits(got, want):
    """Equal bit for bit where `want` is a number, NaN where it is not."""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


# ---- the stand-alone entry
def test_the_stand_alone_entry_equals_the_restatement_bit_for_bit(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    import torch
    cams = _cams(1)
    rng = np.random.default_rng(5)
    rows = []
    for i, cam in enumerate(cams):  # about 2000 points each: the hand-made ones, every whole pixel of a coarse grid, random ones
        v, u = np.mgrid[0:cam["Hs"]:3, 0:cam["Ws"]:3]
        grid = np.stack([u.ravel(), v.ravel()], 1).astype(np.float64)
        rnd = np.stack([rng.uniform(-10, cam["Ws"] + 10, 1400), rng.uniform(-10, cam["Hs"] + 10, 1400)], 1)
        rows.append(np.concatenate([np.array(rref.edge_points(cam)), grid, rnd]))
    rows.insert(1, np.zeros((0, 2)))  # an empty row between them
    row_cams = [cams[0], cams[1], cams[1], api.XI_ABOVE_1]
    rows.append(np.array([(39.5, 29.5), (49.5, 29.5), (60.0, 29.5), (79.0, 29.5), (79.0, 59.0)]))  # solved, solved, lambda - xi < 0, beta < 0 twice
    want = [rref.inverse(c, uv) for c, uv in zip(row_cams, rows)]
    want_xy, want_ok = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert 0 < want[0][1].mean() < 1 and len(rows[0]) > 1900 and len(rows[2]) > 1900  # solved and unsolved points both occur
    xy, ok, off = workloads.undistort_points_batch(gpu_ctx, _pairs_cameras(row_cams), rows)
    torch.cuda.synchronize()
    assert off.tolist() == [0, len(rows[0]), len(rows[0]), len(rows[0]) + len(rows[2]), len(rows[0]) + len(rows[2]) + 5]
    assert want[3][1].tolist() == [1, 1, 0, 0, 0]
    assert _nan_equal_bits(xy.cpu().numpy(), want_xy)
    assert np.array_equal(ok.cpu().numpy(), want_ok)
    again, none, _ = workloads.undistort_points_batch(gpu_ctx, _pairs_cameras(row_cams), rows, want_ok=False)  # d_ok_or_null = NULL
    torch.cuda.synchronize()
    assert none is None and _nan_equal_bits(again.cpu().numpy(), want_xy)


def test_the_stand_alone_entrys_argument_errors(mbavo, gpu_ctx):
    import torch
    capi, lib = mbavo.capi, gpu_ctx.lib
    cams = _pairs_cameras(_cams(1))
    arr = (capi.PairsCamera * 2)(*cams)
    uv = torch.full((10, 2), 20.0, dtype=torch.float64, device="cuda:0")
    xy = torch.full((10, 2), -7.0, dtype=torch.float64, device="cuda:0")
    ip = lambda a: capi.ip(np.ascontiguousarray(a, dtype=np.int32))
    up, xp, good = uv.data_ptr(), xy.data_ptr(), ip([0, 4, 10])
    call = lambda n, cams_, off, u, x: lib.mbavo_undistort_points_batch(gpu_ctx.handle, n, cams_, off, u, x, None)
    assert call(2, None, good, up, xp) == E_ARG and call(2, arr, None, up, xp) == E_ARG
    assert call(2, arr, good, None, xp) == E_ARG and call(2, arr, good, up, None) == E_ARG
    assert call(0, arr, good, up, xp) == E_ARG and call(65536, arr, good, up, xp) == E_ARG and call(-1, arr, good, up, xp) == E_ARG
    assert call(2, arr, ip([0, 6, 4]), up, xp) == E_ARG and call(2, arr, ip([1, 4, 10]), up, xp) == E_ARG
    for field, value in (("model", 3), ("model", 0), ("H", 0), ("xi", -0.5), ("xi", float("nan"))):
        bad = (capi.PairsCamera * 2)(*cams)
        setattr(bad[1], field, value)
        assert call(2, bad, good, up, xp) == E_ARG, field
    for i, j in ((0, 0), (1, 1)):  # fx or fy equal to 0 on either camera
        for name in ("intrinsics", "to_intrinsics"):
            bad = (capi.PairsCamera * 2)(*cams)
            getattr(bad[i], name)[j] = 0.0
            assert call(2, bad, good, up, xp) == E_ARG, (name, j)
    torch.cuda.synchronize()
    assert (xy.cpu().numpy() == -7.0).all()  # nothing was launched
    assert call(2, arr, ip([0, 0, 0]), None, None) == 0  # NULL arrays with an empty total are fine
    assert call(2, arr, good, up, xp) == 0
    torch.cuda.synchronize()
    assert np.isfinite(xy.cpu().numpy()).all()


# ---- the pairs batch
@pytest.mark.parametrize("scale,r", [(1, 2), (1, 0), (2, 2)])
def test_prepare_points_in_the_raw_geometry(mbavo, gpu_ctx, scale, r):
    """Against the restatement's composition, against the stand-alone entry followed by a geometry-0 call on a second object, in
    its statistics against a geometry-0 call on the same object; geometry 0 again gives the bits of a run that never set it."""
    c = _case(scale)
    H, W = c["H"], c["W"]
    clears = _clears(c, r, CAMERA_OF_PAIR)
    want, want_counts = rref.keypoints(c["lists"], c["of_pair"], L, H, W, BORDERS, clears)
    assert (want_counts[2] == 0).all() and all(0 < want_counts[b, l] < c["n"] for b in (0, 1) for l in range(L))
    if r > 0:  # the clearance test bites
        assert (want_counts < rref.keypoints(c["lists"], c["of_pair"], L, H, W, BORDERS)[1]).any()
    pb, two = _object(gpu_ctx, c, r), _object(gpu_ctx, c, r)
    try:
        sharp, blur = dv.dev(c["sharp"], c["blur"])
        as_geometry0 = [(np.ascontiguousarray(uv * (W / c["Ws"])), z) for uv, z in c["lists"]]  # the same numbers read as undistorted points
        never = dv.read_batch(pb, pb.prepare_points(sharp, blur, as_geometry0))
        stats0 = pb.stats()
        assert pb.set_points_geometry(1) == 0
        counts = pb.prepare_points(sharp, blur, c["lists"])
        got = dv.read_batch(pb, counts)
        _assert_keypoints(got, want, counts, want_counts, ("restatement", scale, r))
        assert pb.stats() == stats0 and stats0[:2] == (1 + 3, 1)  # remap, pyramid, gradients, points; one synchronisation
        composed = _composed(gpu_ctx, c["of_pair"], c["lists"])
        assert any(len(q[1]) < len(p[1]) for q, p in zip(composed, c["lists"]))  # points outside the raw image were removed
        cc = two.prepare_points(sharp, blur, composed)
        assert np.array_equal(cc, counts)
        dv.assert_twins(got, dv.read_batch(two, cc), ("composed", scale, r))
        assert two.stats() == stats0
        assert pb.set_points_geometry(0) == 0
        back = pb.prepare_points(sharp, blur, as_geometry0)
        dv.assert_twins(dv.read_batch(pb, back), never, ("geometry 0 again", scale, r))
    finally:
        pb.close()
        two.close()


@pytest.mark.parametrize("one", [None, 0, 1])
def test_update_points_in_the_raw_geometry(mbavo, gpu_ctx, one):
    """n_key = 2, pairs 0 and 2 listed: row i is pair h_key_pairs[i] and goes through that pair's camera; pair 1's keyframe side
    stays.  With the camera set and with either camera alone (mbavo_pairs_set_camera, _set_camera_unified)."""
    c = _case(1)
    H, W, r = c["H"], c["W"], 2
    keys = [0, 2]
    index = list(CAMERA_OF_PAIR) if one is None else [one] * B
    of_pair = [c["cams"][g] for g in index]
    lists0 = [_raw_list(of_pair[b], c["n"], 10 + b) for b in range(B)]
    new_lists = [_raw_list(of_pair[b], 150, 20 + b) for b in keys]
    clears = _clears(c, r, index)
    latest = list(lists0)
    for i, b in enumerate(keys):
        latest[b] = new_lists[i]
    want, want_counts = rref.keypoints(latest, of_pair, L, H, W, BORDERS, clears)
    first_counts = rref.keypoints(lists0, of_pair, L, H, W, BORDERS, clears)[1]
    assert (want_counts > 0).all() and (want_counts[keys] != first_counts[keys]).any(1).all()
    pb, two = _object(gpu_ctx, c, r, one), _object(gpu_ctx, c, r, one)
    try:
        sharp, blur, new_sharp, new_blur = dv.dev(c["sharp"], c["blur"], c["new_sharp"], c["new_blur"])
        for o, lists in ((pb, lists0), (two, _composed(gpu_ctx, of_pair, lists0))):
            o.prepare_points(sharp, blur, lists)  # (pb in geometry 0 for now: the statistics of a geometry-0 update below)
        pb.update_points(new_blur, keys, new_sharp, new_lists)
        stats0 = pb.step_stats()[0]
        assert pb.set_points_geometry(1) == 0
        before = dv.read_batch(pb, pb.prepare_points(sharp, blur, lists0))
        counts = pb.update_points(new_blur, keys, new_sharp, new_lists)
        got = dv.read_batch(pb, counts)
        _assert_keypoints(got, want, counts, want_counts, ("update", one))
        assert pb.step_stats()[0] == stats0
        for e in range(L, 2 * L):  # pair 1 is not listed: its keyframe side has the bytes it had
            assert all(dv.same_bits(got[e][key], before[e][key]) for key in ("ref", "grad", "xy", "z")), e
        assert not dv.same_bits(got[0]["xy"], before[0]["xy"]) and not dv.same_bits(got[2 * L]["xy"], before[2 * L]["xy"])
        cc = two.update_points(new_blur, keys, new_sharp, _composed(gpu_ctx, [of_pair[b] for b in keys], new_lists))
        assert np.array_equal(cc, counts)
        dv.assert_twins(got, dv.read_batch(two, cc), ("update, composed", one))
        assert two.step_stats()[0] == stats0
    finally:
        pb.close()
        two.close()


def test_the_setters_errors(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    c = _case(1)
    lib = gpu_ctx.lib
    pb = _object(gpu_ctx, c, 0)
    flat = workloads.PairBatch(gpu_ctx, B, L=L, H=c["H"], W=c["W"], border=list(BORDERS), cell=0, thresh=3.0, every_candidate=True)
    try:
        sharp, blur = dv.dev(c["sharp"], c["blur"])
        assert pb.set_points_geometry(1) == 0
        held = pb.prepare_points(sharp, blur, c["lists"])
        for bad in (2, -1, 7):
            assert pb.set_points_geometry(bad) == E_ARG
        assert np.array_equal(pb.prepare_points(sharp, blur, c["lists"]), held)  # nothing changed: still raw
        assert lib.mbavo_pairs_set_points_geometry(None, 1) == E_ARG
        # an object that takes pinhole images has no raw camera
        assert flat.set_points_geometry(1) == E_ARG and flat.set_points_geometry(2) == E_ARG and flat.set_points_geometry(0) == 0
        und = dv.dev(np.ascontiguousarray(c["sharp"][:, :c["H"], :c["W"]]), np.ascontiguousarray(c["blur"][:, :c["H"], :c["W"]]))
        plain = [(np.ascontiguousarray(uv * 0.8), z) for uv, z in c["lists"]]
        import pairs_points_ref as pref
        counts = flat.prepare_points(und[0], und[1], plain)
        assert np.array_equal(counts, pref.keypoints(plain, L, c["H"], c["W"], BORDERS)[1])  # geometry 0, as ever
    finally:
        pb.close()
        flat.close()


def test_one_evaluation_runs_on_a_raw_points_object(mbavo, gpu_ctx):
    import torch
    c = _case(1)
    capi, k, N = mbavo.capi, 4, 4
    pb = _object(gpu_ctx, c, 2, borders=(20, 10, 5))  # (every patch inside its level)
    try:
        assert pb.set_points_geometry(1) == 0
        counts = pb.prepare_points(*dv.dev(c["sharp"], c["blur"]), c["full"])
        assert (counts > 0).all()
        rng = np.random.default_rng(2)
        kt = rng.normal(0, 2e-3, (B, N, 3))
        kR = np.tile(np.array([0.0, 0, 0, 1]), (B, N, 1)) + rng.normal(0, 1e-3, (B, N, 4))
        kR /= np.linalg.norm(kR, axis=2, keepdims=True)
        assert pb.set_motion(np.full(B, 0.3), np.full(B, 0.04), np.zeros(B), 0.5, kt, kR) == 0
        n, E = B * L, int(gpu_ctx.lib.mbavo_packed_len(k))
        fb = torch.full((n * E,), float("nan"), dtype=torch.float64, device="cuda:0")
        valid = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        capi.check(gpu_ctx.lib.mbavo_eval_batch(gpu_ctx.handle, n, pb.array, k, 1, fb.data_ptr(), None, valid.data_ptr()), "mbavo_eval_batch")
        torch.cuda.synchronize()
        blocks = fb.cpu().numpy().reshape(n, E)
        assert np.isfinite(blocks).all() and (np.abs(blocks).max(1) > 0).all() and np.isfinite(valid.cpu().numpy()).all()
    finally:
        pb.close()
