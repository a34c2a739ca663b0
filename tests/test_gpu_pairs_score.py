"""mbavo_pairs_set_detector on plain pairs objects: after a prepare, an update and a track_frame under the corner score the object
holds the keypoints of the restated selection (tests/pairs_score_ref.py: the host detector of the other pairs tests with the
response swapped) bit for bit -- counts, every (x, y, z), the order -- under grid selection and under every_candidate = 1, with
keyframe formats 0 and 2, at 64 x 80 and 65 x 67 (levels 65/32/16 by 67/33/16) with 8 x 8 cells; the launch statistics show the
one launch more (none more without a key list); a return to score 0 gives the bytes and statistics of a twin that never asked;
rejected options change nothing; a vertical step edge, the aperture case, has no keypoint under the score and some under the
gradient magnitude.

Each pair gets its own texture with a band of vertical stripes (straight edges: picks under the gradient magnitude, none under the
score), a flat band and a depth map with holes, so that the counts differ per pair and level."""
import ctypes as C

import numpy as np
import pytest

import pairs_device as dv
import pairs_score_ref as sr
import pairs_step as ps
from lm_support import lm_batch_opts
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
B, L, CELL = 3, 3, 8
BORDER = (3, 2, 1)
THR_SCORE, THR_GRAD = 2.0, 4.0
CONFIGS = [(H_, W_, dense_, fmt_) for H_, W_ in ((64, 80), (65, 67)) for dense_ in (False, True) for fmt_ in (0, 2)]
_INPUTS = {}


def _image(H, W, seed, b):
    img = synth.texture_image(H, W, seed=seed, octaves=(8, 4)).copy()
    y, x = np.mgrid[0:H, 0:W]
    x0 = 8 + 14 * b
    band = (x >= x0) & (x < x0 + 18)
    img[band] = np.where((x // 3) % 2 == 0, 60, 190).astype(np.uint8)[band]  # vertical stripes: ky = 0 inside the band
    img[H - 14 - 5 * b:H - 4 - 5 * b, :] = 128                                 # a flat band
    return img


def inputs(H, W):
    """Made once per size and left unchanged: sharp / blur / depth of B pairs, a second keyframe for pair 1, later current frames."""
    if (H, W) not in _INPUTS:
        rng = np.random.default_rng(H * W)
        sharp = np.stack([_image(H, W, 11 + 7 * b, b) for b in range(B)])
        depth = rng.uniform(0.8, 3.0, (B, H, W)).astype(np.float32)
        depth[rng.uniform(0, 1, depth.shape) < 0.12] = 0.0
        blur = np.stack([np.roll(s, (1, -2), (0, 1)) for s in sharp])
        c = dict(sharp=sharp, depth=depth, blur=np.ascontiguousarray(blur), new_sharp=_image(H, W, 301, 2)[None].copy(),
                 new_depth=rng.uniform(0.8, 3.0, (1, H, W)).astype(np.float32), new_blur=np.ascontiguousarray(np.roll(blur, (2, 1), (1, 2))),
                 blur3=np.ascontiguousarray(np.roll(blur, (-1, 3), (1, 2))))
        for v in c.values():
            v.setflags(write=False)
        _INPUTS[(H, W)] = c
    return _INPUTS[(H, W)]


def batch(ctx, H, W, dense, fmt, thresh=THR_GRAD):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=3, k=2, N=2, cell=CELL, thresh=thresh, border=list(BORDER), keyframe_format=fmt,
                               every_candidate=dense)


def restated(sharp, depth, H, W, dense, r, thr):
    """Per (pair, level): (xy, z) of the restated selection; r = 0: by gradient magnitude."""
    out = []
    for b in range(len(sharp)):
        for l, im in enumerate(synth.pyramid(np.ascontiguousarray(sharp[b]), L)):
            out.append(sr.keypoints(im, l, H, W, CELL, thr, depth[b], BORDER[l], r, dense))
    return out


def assert_keypoints(got, want, counts, tag):
    assert len(got) == len(want)
    for e, (g, (xy, z)) in enumerate(zip(got, want)):
        assert counts.ravel()[e] == len(z), (tag, e, int(counts.ravel()[e]), len(z))
        assert np.array_equal(g["xy"], xy) and np.array_equal(g["z"], z), (tag, e)


def held_bytes(H, W, fmt):
    gb = 8 if fmt == 0 else 4
    px = sum(((H >> l) * (W >> l) + 15) // 16 * 16 for l in range(L))
    return B * ((px * gb + 255) // 256 * 256 // gb) * 4


def dev_all(c):
    return {k: (dv.dev_depth(np.array(v)) if "depth" in k else dv.dev(np.array(v))[0]) for k, v in c.items()}  # (copies: the inputs are read-only)


@pytest.mark.parametrize("H,W,dense,fmt", CONFIGS)
def test_prepare_update_and_back(mbavo, gpu_ctx, H, W, dense, fmt):
    c = inputs(H, W)
    t = dev_all(c)
    twin, pb = batch(gpu_ctx, H, W, dense, fmt), batch(gpu_ctx, H, W, dense, fmt)
    try:
        # the twin never calls set_detector
        counts0 = twin.prepare(t["sharp"], t["depth"], t["blur"])
        plain, stats0 = dv.read_batch(twin, counts0), twin.stats()
        assert_keypoints(plain, restated(c["sharp"], c["depth"], H, W, dense, 0, THR_GRAD), counts0, "gradient magnitude")
        twin.update(t["new_blur"], [1], t["new_sharp"], t["new_depth"])
        upd0 = twin.step_stats()[0]
        twin.update(t["blur3"])
        upd0_nokey = twin.step_stats()[0]
        # rejected options: the mode stays, nothing is allocated
        assert pb.detector_stats() == (0, 0, 0)
        bad = [dict(score=1, radius=0, threshold=1.0), dict(score=1, radius=4, threshold=1.0), dict(score=1, radius=2, threshold=float("nan")),
               dict(score=1, radius=2, threshold=-1.0), dict(score=2, radius=2, threshold=1.0), dict(score=1, radius=2, threshold=1.0, reserved=[0, 0, 7]),
               dict(score=0, reserved=[1])]
        for kw in bad:
            assert pb.set_detector(**kw) == E_ARG, kw
        assert pb.detector_stats() == (0, 0, 0)
        # r = 1
        assert pb.set_detector(1, 1, THR_SCORE) == 0
        held = held_bytes(H, W, fmt)
        assert pb.detector_stats() == (1, 1, held)
        counts = pb.prepare(t["sharp"], t["depth"], t["blur"])
        got = dv.read_batch(pb, counts)
        want1 = restated(c["sharp"], c["depth"], H, W, dense, 1, THR_SCORE)
        assert_keypoints(got, want1, counts, "r = 1")
        assert pb.stats() == (stats0[0] + 1,) + stats0[1:]
        for g, p in zip(got, plain):  # images and gradients are those of the twin
            assert all(dv.same_bits(g[k], p[k]) for k in ("ref", "cur", "grad"))
        assert len({len(z) for _, z in want1}) > L and any(len(w[1]) != len(p["z"]) for w, p in zip(want1, plain))
        before_bad = (pb.stats(), pb.step_stats())
        for kw in bad:
            assert pb.set_detector(**kw) == E_ARG, kw
        assert pb.detector_stats() == (1, 1, held)
        assert (pb.stats(), pb.step_stats()) == before_bad  # (no call's statistics moved; that the call holds no launch at all is
        #                                                      asserted on its source by tests/test_pairs_score_api.py)
        counts_again = pb.prepare(t["sharp"], t["depth"], t["blur"])
        assert_keypoints(dv.read_batch(pb, counts_again), want1, counts_again, "r = 1 after the rejected calls")  # the mode held
        assert pb.stats() == (stats0[0] + 1,) + stats0[1:]
        # r = 3
        assert pb.set_detector(1, 3, THR_SCORE) == 0 and pb.detector_stats() == (1, 3, held)
        counts = pb.prepare(t["sharp"], t["depth"], t["blur"])
        before = dv.read_batch(pb, counts)
        want3 = restated(c["sharp"], c["depth"], H, W, dense, 3, THR_SCORE)
        assert_keypoints(before, want3, counts, "r = 3")
        assert any(not np.array_equal(a[0], b_[0]) for a, b_ in zip(want1, want3))
        # an update with a key list of one pair re-detects that pair alone, one launch more
        counts = pb.update(t["new_blur"], [1], t["new_sharp"], t["new_depth"])
        after = dv.read_batch(pb, counts)
        new1 = restated(c["new_sharp"], c["new_depth"], H, W, dense, 3, THR_SCORE)
        assert_keypoints(after[L:2 * L], new1, counts[1], "update: the listed pair")
        for e in list(range(L)) + list(range(2 * L, 3 * L)):
            assert all(dv.same_bits(after[e][k], before[e][k]) for k in ("ref", "grad", "xy", "z")), ("update: the other pairs", e)
        assert pb.step_stats()[0] == (upd0[0] + 1,) + upd0[1:]
        # without a key list: none more
        pb.update(t["blur3"])
        assert pb.step_stats()[0] == upd0_nokey
        # back to the default: a twin's bytes and statistics, the slices still held
        assert pb.set_detector(None) == 0 and pb.detector_stats() == (0, 0, held)
        counts = pb.prepare(t["sharp"], t["depth"], t["blur"])
        assert counts.tolist() == counts0.tolist()
        dv.assert_twins(dv.read_batch(pb, counts), plain, "back to score 0")
        assert pb.stats() == stats0
        pb.update(t["new_blur"], [1], t["new_sharp"], t["new_depth"])
        assert pb.step_stats()[0] == upd0
    finally:
        pb.close()
        twin.close()


@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_track_frame_equals_the_composed_calls(mbavo, gpu_ctx, dense, fmt):
    """One track_frame with a keyframe switch of pair 1 under the score against update, predict, mbavo_lm_batch_levels and commit by
    hand on a twin: the same arrays, counts and verdicts, and the restated keypoints for the new keyframe."""
    import torch
    H, W, capi = 65, 67, mbavo.capi
    c = inputs(H, W)
    t = dev_all(c)
    one, two = batch(gpu_ctx, H, W, dense, fmt), batch(gpu_ctx, H, W, dense, fmt)
    try:
        for pb in (one, two):
            assert pb.set_detector(1, 2, THR_SCORE) == 0
            pb.prepare(t["sharp"], t["depth"], t["blur"])
            assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
        cap, exp, opts = np.full(B, 0.1), np.full(B, 0.02), lm_batch_opts(capi, 2, 3)
        thr = (ps.FLOW0, ps.FLOW1, ps.KERNEL)
        frames, counts, res, _ = one.track_frame(t["new_blur"], cap, exp, opts, thr, [1], t["new_sharp"], t["new_depth"])
        assert one.step_stats()[0][0] > 0
        counts2 = two.update(t["new_blur"], [1], t["new_sharp"], t["new_depth"])
        assert two.step_stats()[0] == one.step_stats()[0]
        assert two.predict(cap, exp) == 0
        res2 = (capi.LmBatchResult * B)()
        assert gpu_ctx.lib.mbavo_lm_batch_levels(gpu_ctx.handle, B, L, two.array, C.byref(opts), res2, None, 0) == 0
        frames2 = two.commit(*thr)
        torch.cuda.synchronize()
        assert counts.tolist() == counts2.tolist()
        dv.assert_twins(dv.read_batch(one, counts), dv.read_batch(two, counts2), "track_frame against the composed calls")
        # (the frames' verdicts and keypoint counts; the poses are the LM's business, which test_gpu_pairs_track.py compares)
        assert [(f.a.status, f.a.is_keyframe, f.a.num_keypoints0) for f in frames] == [(f.a.status, f.a.is_keyframe, f.a.num_keypoints0) for f in frames2]
        assert [f.a.num_keypoints0 for f in frames] == counts[:, 0].tolist()
        assert_keypoints(dv.read_batch(one, counts)[L:2 * L], restated(c["new_sharp"], c["new_depth"], H, W, dense, 2, THR_SCORE), counts[1],
                         "track_frame: the new keyframe")
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("dense", [False, True])
def test_a_straight_edge_has_no_keypoint_under_the_score(mbavo, gpu_ctx, dense):
    """The aperture case, exact by the identity ky = 0: K = 0 on every level under score = 1 with a positive threshold, K > 0 under
    score = 0."""
    H, W = 64, 80
    x = np.mgrid[0:H, 0:W][1]
    sharp = np.ascontiguousarray(np.broadcast_to(np.where(x >= W // 2, 200, 30).astype(np.uint8), (B, H, W)))
    ts, td = dv.dev(sharp, np.ones((B, H, W), np.float32))
    pb = batch(gpu_ctx, H, W, dense, 0, thresh=THR_GRAD)
    try:
        assert (pb.prepare(ts, td, ts) > 0).all()
        assert pb.set_detector(1, 2, 0.25) == 0
        assert not pb.prepare(ts, td, ts).any()
        assert pb.set_detector(0) == 0
        assert (pb.prepare(ts, td, ts) > 0).all()
    finally:
        pb.close()
