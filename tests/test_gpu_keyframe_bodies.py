"""The device bodies that the per-image kernels (image_ops.hip, keyframe_ops.hip) and the batched ones (pairs_prep.hip) both call
from keyframe_math.h, at the sizes where each can go wrong, against the numpy restatements (tests/pairs_ref.py,
tests/pairs_dense_ref.py, synth.pyramid, synth.pack_keyframe).  Every comparison is exact.

  workgroup prefix sums   256 items are one chunk of the scan, 257 or 272 a full chunk and a ragged second: grid selection with
                          cell 8 on 120 x 120 (16 x 16 cells) and 120 x 128 (16 x 17); every candidate over 256 and 257 rows
                          (per image) and over 256 and 257 segments of 256 pixels (batched: 256 x 256 and 256 x 257)
  pyramid tile            75 x 101 with four levels: 37 x 50, 18 x 25, 9 x 12 -- every level drops an odd row or column
  pixel differences       75 x 101 = 7575 pixels, no multiple of 4: the batched walk's last lane is ragged, its pad stays zero"""
import ctypes as C

import numpy as np
import pytest

import pairs_dense_ref as dref
import pairs_device as dv
import pairs_ref
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

CELL, THR = 8, 4.0
SENTINEL = -7.0


def _inputs(H, W, seed):
    """A textured image with a flat patch (grid cells and whole rows without a candidate) and a depth map with holes."""
    rng = np.random.default_rng(seed)
    img = synth.texture_image(H, W, seed=seed, octaves=(16, 8, 4))
    img[24:64, :] = 128
    depth = rng.uniform(0.5, 3.0, (H, W)).astype(np.float32)
    depth[rng.uniform(0, 1, (H, W)) < 0.15] = 0.0
    return img, depth


def _want(img, depth, cell):
    """The restatement's keypoints of level 0 without a border, and that they are worth comparing."""
    H, W = img.shape
    if cell:
        xy, z = pairs_ref.keypoints(img, 0, H, W, cell, cell, THR, depth, 0)
        picks = pairs_ref.picks(pairs_ref.gradient_magnitude(img), 0, H, W, cell, cell, THR)
        inside = [p for ci, p in enumerate(picks) if (ci // (W // cell + 1) + 1) * cell <= H and (ci % (W // cell + 1) + 1) * cell <= W]
        assert None in inside and any(p is not None for p in inside)  # empty cells inside the image, between kept ones
    else:
        xy, z = dref.keypoints(img, 0, THR, depth, 0)
        rows = np.bincount(xy[:, 1].astype(np.int64), minlength=H)
        assert (rows[1:-1] == 0).any() and rows[-2] > 0  # rows without a candidate; the last scanned row has some
    assert len(z) > 4
    return xy, z


def _detect(ctx, capi, img, depth, cell, cap, size):
    """mbavo_detect_semidense on level 0 into sentinel-filled arrays of `size` keypoints: (count, xy, z)."""
    import torch
    H, W = img.shape
    ti, td = dv.dev(img, depth)
    xy = torch.full((2 * size,), SENTINEL, dtype=torch.float64, device="cuda:0")
    kz = torch.full((size,), SENTINEL, dtype=torch.float64, device="cuda:0")
    cnt = C.c_int(-1)
    capi.check(ctx.lib.mbavo_detect_semidense(ctx.handle, ti.data_ptr(), H, W, 0, H, W, cell, cell, THR, td.data_ptr(), xy.data_ptr(),
                                              kz.data_ptr(), cap, C.byref(cnt)), "mbavo_detect_semidense")
    return cnt.value, xy.cpu().numpy().reshape(-1, 2), kz.cpu().numpy()


@pytest.mark.parametrize("cell,H,W", [(CELL, 120, 120), (CELL, 120, 128), (0, 256, 70), (0, 257, 70)])
def test_per_image_compaction_at_a_chunk_boundary(mbavo, gpu_ctx, cell, H, W):
    """Count and arrays of mbavo_detect_semidense; with cap = K // 2 the same count, the first cap keypoints, nothing behind them."""
    img, depth = _inputs(H, W, seed=H + W)
    if cell:
        assert pairs_ref.cells_per_level(H, W, 1, cell, cell)[0] == {120: 256, 128: 272}[W]
    wxy, wz = _want(img, depth, cell)
    K = len(wz)
    for cap in (K, K // 2):
        n, xy, z = _detect(gpu_ctx, mbavo.capi, img, depth, cell, cap, K + 8)
        assert n == K
        assert np.array_equal(xy[:cap], wxy[:cap]) and np.array_equal(z[:cap], wz[:cap])
        assert np.all(xy[cap:] == SENTINEL) and np.all(z[cap:] == SENTINEL)


def _batch(ctx, L, H, W, **kw):
    from mba_vo_amd import workloads
    return workloads.PairBatch(ctx, 2, L=L, H=H, W=W, border=0, cell=CELL, thresh=THR, **kw)


@pytest.mark.parametrize("dense,H,W", [(False, 120, 120), (False, 120, 128), (True, 256, 256), (True, 256, 257)])
def test_batched_compaction_at_a_chunk_boundary(mbavo, gpu_ctx, dense, H, W):
    """mbavo_pairs_prepare, B = 2, L = 1, a different image per pair: counts and keypoints against the restatement."""
    if dense:
        assert (H * W + 255) // 256 == {256: 256, 257: 257}[W]
    pairs = [_inputs(H, W, seed=H + W + 50 * b) for b in range(2)]
    sharp, depth = (np.ascontiguousarray(np.stack([p[i] for p in pairs])) for i in (0, 1))
    want = [_want(img, d, 0 if dense else CELL) for img, d in pairs]
    assert not np.array_equal(want[0][0], want[1][0])
    pb = _batch(gpu_ctx, 1, H, W, every_candidate=dense)
    try:
        counts = pb.prepare(*dv.dev(sharp, depth, np.ascontiguousarray(sharp[::-1])))
        got = dv.read_batch(pb, counts)
        assert counts.ravel().tolist() == [len(w[1]) for w in want]
        for g, w in zip(got, want):
            assert np.array_equal(g["xy"], w[0]) and np.array_equal(g["z"], w[1])
    finally:
        pb.close()


RAGGED = (75, 101, 4)  # 37 x 50, 18 x 25, 9 x 12
_RAGGED = {}


def _ragged():
    """Two images of the ragged size with their numpy pyramids, made once."""
    if not _RAGGED:
        H, W, L = RAGGED
        imgs = [synth.texture_image(H, W, seed=s, octaves=(16, 8, 4)) for s in (3, 4)]
        pyrs = [synth.pyramid(im, L) for im in imgs]
        assert [p.shape for p in pyrs[0]] == [(75, 101), (37, 50), (18, 25), (9, 12)] and all(p.std() > 0 for q in pyrs for p in q)
        _RAGGED.update(imgs=imgs, pyrs=pyrs)
    return _RAGGED["imgs"], _RAGGED["pyrs"]


def _gradients(img, fmt):
    """A level's gradient image in keyframe format `fmt`, as bytes."""
    if fmt == 2:
        return synth.pack_keyframe(img).view(np.uint8).ravel()
    f = img.astype(np.float32)
    g = np.zeros(img.shape + (2,), np.float32)
    g[1:-1, 1:-1, 0] = np.float32(0.5) * (f[1:-1, 2:] - f[1:-1, :-2])
    g[1:-1, 1:-1, 1] = np.float32(0.5) * (f[2:, 1:-1] - f[:-2, 1:-1])
    assert np.abs(g).max() > 0
    return (g if fmt == 0 else g.astype(np.float16)).view(np.uint8).ravel()


def test_pyramid_tile_at_ragged_edges(mbavo, gpu_ctx):
    """mbavo_pyramid_levels_u8 and both images of every pair of a B = 2 prepare against synth.pyramid."""
    import torch
    H, W, L = RAGGED
    imgs, pyrs = _ragged()
    for img, pyr in zip(imgs, pyrs):
        lv = [dv.dev(img.ravel())[0]] + [torch.full(((H >> l) * (W >> l) + 8,), 0xA5, dtype=torch.uint8, device="cuda:0") for l in range(1, L)]
        ptrs = (C.c_void_p * L)(*[a.data_ptr() for a in lv])
        mbavo.capi.check(gpu_ctx.lib.mbavo_pyramid_levels_u8(gpu_ctx.handle, ptrs, H, W, L), "mbavo_pyramid_levels_u8")
        for l in range(1, L):
            got = lv[l].cpu().numpy()
            assert np.array_equal(got[:-8], pyr[l].ravel()) and np.all(got[-8:] == 0xA5), l  # nothing behind the level
    pb = _batch(gpu_ctx, L, H, W)
    try:
        sharp, blur = np.ascontiguousarray(np.stack(imgs)), np.ascontiguousarray(np.stack(imgs[::-1]))
        got = dv.read_batch(pb, pb.prepare(*dv.dev(sharp, np.ones((2, H, W), np.float32), blur)))
        for e, g in enumerate(got):
            b, l = divmod(e, L)
            assert np.array_equal(g["ref"], pyrs[b][l].ravel()) and np.array_equal(g["cur"], pyrs[1 - b][l].ravel()), e
    finally:
        pb.close()


def test_gradients_at_an_odd_pixel_count(mbavo, gpu_ctx):
    """The three per-image producers on 75 x 101 against numpy, and every level of a B = 2 prepare in the three keyframe formats
    against numpy, with the pad behind the level (to a multiple of 16 pixels) still zero."""
    import torch
    H, W, L = RAGGED
    imgs, pyrs = _ragged()
    lib, capi = gpu_ctx.lib, mbavo.capi
    ti = dv.dev(imgs[0])[0]
    n = H * W
    assert n % 4 == 3
    entries = (lib.mbavo_image_gradients_u8, lib.mbavo_image_gradients_u8_half, lib.mbavo_pack_keyframe_u8)
    for fmt, entry in enumerate(entries):
        gb = 8 if fmt == 0 else 4
        out = torch.full((n * gb + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        capi.check(entry(ti.data_ptr(), H, W, out.data_ptr(), None), "gradients, format %d" % fmt)
        got = out.cpu().numpy()
        assert np.array_equal(got[:-16], _gradients(imgs[0], fmt)) and np.all(got[-16:] == 0xA5), fmt
    sharp, blur = np.ascontiguousarray(np.stack(imgs)), np.ascontiguousarray(np.stack(imgs[::-1]))
    for fmt in range(3):
        gb = 8 if fmt == 0 else 4
        pb = _batch(gpu_ctx, L, H, W, keyframe_format=fmt)
        try:
            pb.prepare(*dv.dev(sharp, np.ones((2, H, W), np.float32), blur))
            for e in range(2 * L):
                b, l = divmod(e, L)
                nl = (H >> l) * (W >> l)
                padded = (nl + 15) // 16 * 16
                got = dv.peek(pb.array[e].d_ref_dIxy, padded * gb, np.uint8)
                assert np.array_equal(got[:nl * gb], _gradients(pyrs[b][l], fmt)), (fmt, e)
                assert padded > nl and not got[nl * gb:].any(), (fmt, e)
        finally:
            pb.close()
