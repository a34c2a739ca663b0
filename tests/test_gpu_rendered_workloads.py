"""The rendered workloads (mba_vo_amd.workloads): RenderedPairBatch and RenderedPairPyramids stand on one RenderedScene and one pair
renderer, so level 0 of the pyramids IS the batch, bit for bit -- what the tests that hold the pairs batch to the per-image path
rely on.  Everything is read through the objects' own mbavo_problem arrays (the pointers a consumer gets).  At level 0 the two
classes' borders (20), keypoint capacities and detector arguments coincide: every comparison is exact.  One test needs no GPU: the
scene's host part."""
import ctypes as C

import numpy as np
import pytest

import pairs_device as dv
import pairs_ref
from mba_vo_amd import synth, workloads as wl

B, L, H, W, SEED = 3, 3, 240, 320, 5
CELL, THR, BORDER0 = 30, 4.0, 20  # the defaults of both classes; the border of level 0
_OBJECTS = {}


def _objects(ctx):
    """The batch and the pyramids of the same three pairs, rendered once for all tests."""
    if not _OBJECTS:
        _OBJECTS["batch"] = wl.RenderedPairBatch(ctx, B, H=H, W=W, seed=SEED)
        _OBJECTS["pyramids"] = wl.RenderedPairPyramids(ctx, B, L=L, H=H, W=W, seed=SEED)
    return _OBJECTS["batch"], _OBJECTS["pyramids"]


def _entry(q):
    """Everything one mbavo_problem with float gradients holds or points at."""
    n = q.H * q.W
    cur = int(dv.peek(q.d_cur_imgs, 1, np.uint64)[0])
    return dict(scalars=(q.S, q.F, q.K, q.P, q.N, q.H, q.W, q.kp_stride, q.num_bad, q.t0, q.dt, q.huber_a, q.grad_fp16, q.h_start_idx[0]),
                intrinsics=list(q.intrinsics), ref=dv.peek(q.d_ref_img, n, np.uint8), cur=dv.peek(cur, n, np.uint8),
                grad=dv.peek(q.d_ref_dIxy, 2 * n, np.float32), xy=dv.peek(q.d_kp_xy, 2 * q.K, np.float64), z=dv.peek(q.d_kp_z, q.K, np.float64),
                pattern=dv.peek(q.d_pattern, 2 * q.P, np.int32), kt=dv.peek(q.d_knots_t, 3 * q.N, np.float64),
                kR=dv.peek(q.d_knots_R, 4 * q.N, np.float64), cap=dv.peek(q.d_cap_time, 1, np.float64), exp=dv.peek(q.d_exp_time, 1, np.float64))


def _assert_entries_equal(a, b, tag):
    assert a.keys() == b.keys()
    for name in a:
        same = np.array_equal(a[name], b[name]) if isinstance(a[name], np.ndarray) else a[name] == b[name]
        assert same, (tag, name)


def test_scene_host_part_does_not_depend_on_what_is_rendered():
    """No GPU.  Pair b's perturbation is the b-th draw of the seed, its times and spline segment depend on b alone: a scene of
    three pairs holds the first three pairs of a scene of six (what `pairs=` and the sharded benches rely on).  Up to the
    benchmark's 512 pairs no exposure straddles a knot and every start index is 0."""
    args = (240, 320, "cpu", SEED, 7.5, 0.1, 0.04, 2e-3)
    short, full = wl.RenderedScene(None, 3, *args), wl.RenderedScene(None, 6, *args)
    rng = np.random.default_rng(SEED)
    for b in range(6):
        draw = rng.normal(0, 2e-3, (4, 3))
        assert np.array_equal(full.perts[b], draw)
        if b < 3:
            assert np.array_equal(short.perts[b], draw)
            assert short.times(b) == full.times(b) == (0.55 + b * 0.1, 0.55 + (b + 1) * 0.1) and short.segment(b) == full.segment(b)
    assert len(short.perts) == 3 and not np.array_equal(full.perts[0], full.perts[1])
    assert np.array_equal(short.intr, [160.0, 160.0, 160.0, 120.0])
    big = wl.RenderedScene(None, 512, *args)
    n = short.n_world  # (the world spline of a longer sequence begins with the shorter's)
    assert n < big.n_world and np.array_equal(short.kt_w, big.kt_w[:n]) and np.array_equal(short.kR_w, big.kR_w[:n])
    for b in range(512):
        idx, tc = big.segment(b), big.times(b)[1]
        t0 = idx * 0.5
        assert t0 <= tc - 0.02 and tc + 0.02 < t0 + 0.5 and idx + 4 <= big.n_world
        assert synth.segment_start_index(tc, t0, 0.5) == 0


@pytest.mark.gpu
def test_level0_of_the_pyramids_is_the_batch(mbavo, gpu_ctx):
    """Every pair: the batch's entry and the pyramids' level-0 entry hold the same keyframe, current image, float gradients, K,
    keypoints, depths, initial knots, times, t0 and intrinsics, bit for bit; so do the named per-pair records."""
    batch, rpp = _objects(gpu_ctx)
    entries = []
    for b in range(B):
        eb, ep = _entry(batch.array[b]), _entry(rpp.array[b * L])
        _assert_entries_equal(eb, ep, b)
        assert eb["scalars"][2] == batch.probs[b].K > 20 and eb["intrinsics"] == [W / 2.0, W / 2.0, W / 2.0, H / 2.0]
        pb, pp = batch.pair(b), rpp.pair(b)
        for name in ("pk", "qk", "kt", "kR", "kt_gt"):
            assert np.array_equal(getattr(pb, name), getattr(pp, name)), (b, name)
        assert (pb.t0, pb.cap, pb.exp) == (pp.t0, pp.cap, pp.exp) == (eb["scalars"][9], eb["cap"][0], eb["exp"][0])
        assert np.array_equal(eb["kt"], pb.kt.ravel()) and np.array_equal(eb["kR"], pb.kR.ravel())
        assert np.array_equal(pb.depth.cpu().numpy(), pp.depth.cpu().numpy())
        assert len(pb.levels) == 1 and len(pp.levels) == L and pb.levels[0].K == pp.levels[0].K == eb["scalars"][2]
        entries.append(eb)
    # not vacuous: the pairs differ from one another
    assert not np.array_equal(entries[0]["ref"], entries[1]["ref"]) and not np.array_equal(entries[0]["kt"], entries[2]["kt"])
    # the coarser levels: half the size and intrinsics per level, the pair's times and knot buffers shared
    for b in range(B):
        for l in range(1, L):
            q, q0, lv = rpp.array[b * L + l], rpp.array[b * L], rpp.pair(b).levels[l]
            assert (q.H, q.W, q.K) == (H >> l, W >> l, lv.K) == (lv.H, lv.W, lv.K) and q.d_ref_img == lv.ref.data_ptr()
            assert list(q.intrinsics) == [v / (1 << l) for v in q0.intrinsics]
            assert (q.d_knots_t, q.d_knots_R, q.d_cap_time, q.d_exp_time) == (q0.d_knots_t, q0.d_knots_R, q0.d_cap_time, q0.d_exp_time)


@pytest.mark.gpu
def test_rendered_inputs_are_what_the_problem_array_holds(mbavo, gpu_ctx):
    """rendered_inputs(rpp): sharp[b] and blur[b] are the bytes behind array[b * L].d_ref_img and the pointer stored in d_cur_imgs;
    depth[b] is the map the detector was given: mbavo_detect_semidense on level 0 with it, then the border filter, gives the
    entry's keypoints and depths again, and every depth is the map's value at its keypoint."""
    import torch
    _, rpp = _objects(gpu_ctx)
    sharp, depth, blur = wl.rendered_inputs(rpp)
    assert sharp.dtype == blur.dtype == torch.uint8 and depth.dtype == torch.float32
    assert tuple(sharp.shape) == tuple(depth.shape) == tuple(blur.shape) == (B, H, W)
    cap = (H // CELL + 1) * (W // CELL + 1)
    for b in range(B):
        q = rpp.array[b * L]
        assert np.array_equal(sharp[b].cpu().numpy().ravel(), dv.peek(q.d_ref_img, H * W, np.uint8))
        assert np.array_equal(blur[b].cpu().numpy().ravel(), dv.peek(int(dv.peek(q.d_cur_imgs, 1, np.uint64)[0]), H * W, np.uint8))
        xy = torch.zeros(cap * 2, dtype=torch.float64, device="cuda:0")
        kz = torch.zeros(cap, dtype=torch.float64, device="cuda:0")
        cnt = C.c_int(0)
        mbavo.capi.check(gpu_ctx.lib.mbavo_detect_semidense(gpu_ctx.handle, sharp[b].data_ptr(), H, W, 0, H, W, CELL, CELL, THR, depth[b].data_ptr(),
                                                            xy.data_ptr(), kz.data_ptr(), cap, C.byref(cnt)), "mbavo_detect_semidense")
        raw = cnt.value
        assert q.K <= raw <= cap
        fxy, fz = pairs_ref.border_filter(xy.cpu().numpy()[:2 * raw].reshape(-1, 2), kz.cpu().numpy()[:raw], H, W, BORDER0)
        assert len(fz) == q.K
        assert np.array_equal(fxy.ravel(), dv.peek(q.d_kp_xy, 2 * q.K, np.float64)) and np.array_equal(fz, dv.peek(q.d_kp_z, q.K, np.float64))
        d = depth[b].cpu().numpy()
        assert np.array_equal(fz, d[(fxy[:, 1] + 0.5).astype(int), (fxy[:, 0] + 0.5).astype(int)].astype(np.float64))


@pytest.mark.gpu
def test_a_pair_rendered_alone_is_the_pair_of_the_whole_batch(mbavo, gpu_ctx):
    """pairs=[2] of B = 3: entry 2 equals entry 2 of the object that rendered all three, perturbation included; the other
    entries stay zero-filled and have no record."""
    batch, _ = _objects(gpu_ctx)
    alone = wl.RenderedPairBatch(gpu_ctx, B, H=H, W=W, seed=SEED, pairs=[2])
    _assert_entries_equal(_entry(alone.array[2]), _entry(batch.array[2]), "alone")
    assert np.array_equal(alone.pair(2).kt - alone.pair(2).kt_gt, batch.pair(2).kt - batch.pair(2).kt_gt)
    assert np.abs(alone.pair(2).kt - alone.pair(2).kt_gt).max() > 0
    for b in (0, 1):
        assert alone.pair(b) is None and not alone.array[b].d_ref_img and alone.array[b].K == 0 and alone.probs[b].K == 0
    assert alone.probs[2].K == batch.probs[2].K
