"""mbavo_corner_score_u8 against the numpy restatement (tests/pairs_score_ref.py), bit for bit, for r = 1, 2, 3.

The kernel takes a level in tiles of 16 rows x 32 columns with a halo of r + 1 pixels.  Sizes: 8 x 8 (smaller than any tile), 3 x 70
(every pixel on or next to the border, three tiles in a row), 9 x 70, 33 x 65 (ragged on both tile edges with an odd width), 64 x
80 (whole tiles in height, ragged in width), 17 x 33 (exactly one tile plus one pixel in each direction).  Contents: random bytes,
a constant, a vertical step, a diagonal step, the 0/255 checkerboard.  The output lies inside a band of NaN that must still be NaN
afterwards, at 0, 4 and 12 bytes from a 16-byte boundary; the source also one byte off."""
import numpy as np
import pytest

import pairs_score_ref as sr

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (3, 70), (9, 70), (33, 65), (64, 80), (17, 33)]
GUARD = 64  # floats of NaN before and after the output
_WANT = {}


def want(H, W, kind, r):
    """The restated score, computed once per case and left unchanged."""
    key = (H, W, kind, r)
    if key not in _WANT:
        w = sr.score(sr.images(H, W, seed=H * 100 + W)[kind], r)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def device_score(ctx, img, r, out_off=0, src_off=0):
    """The device's H x W scores through a source src_off bytes and an output out_off floats off their aligned starts; asserts the
    guard band."""
    import torch
    H, W = img.shape
    src = torch.zeros(H * W + 16, dtype=torch.uint8, device="cuda:0")
    src[src_off:src_off + H * W] = torch.from_numpy(np.ascontiguousarray(img).ravel()).to("cuda:0")
    out = torch.full((2 * GUARD + H * W + 8,), float("nan"), dtype=torch.float32, device="cuda:0")
    assert out.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    first = GUARD + out_off
    rc = ctx.lib.mbavo_corner_score_u8(src.data_ptr() + src_off, H, W, r, out.data_ptr() + 4 * first, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:first]).all() and np.isnan(got[first + H * W:]).all(), "the guard band was written"
    return got[first:first + H * W].reshape(H, W)


def same(got, w, tag):
    assert got.dtype == w.dtype == np.float32
    bad = np.argwhere(got.view(np.uint32) != w.view(np.uint32))
    assert len(bad) == 0, (tag, len(bad), bad[:4].tolist(), [(float(got[y, x]), float(w[y, x])) for y, x in bad[:4]])


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_scores_bit_for_bit(mbavo, gpu_ctx, H, W, r):
    for kind in ("random", "constant", "vstep", "dstep", "checker"):
        same(device_score(gpu_ctx, sr.images(H, W, seed=H * 100 + W)[kind], r), want(H, W, kind, r), (H, W, kind, r))
    assert want(H, W, "random", r).max() > 0
    assert not want(H, W, "constant", r).any() and not want(H, W, "vstep", r).any()  # the exact zeros of the definition


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("out_off,src_off", [(1, 0), (3, 0), (0, 1), (3, 1)])
def test_unaligned_pointers(mbavo, gpu_ctx, r, out_off, src_off):
    """Output 4 and 12 bytes off a 16-byte boundary, source one byte off: the same bits, the guard band untouched."""
    for H, W in ((33, 65), (17, 33)):
        img = sr.images(H, W, seed=H * 100 + W)["random"]
        same(device_score(gpu_ctx, img, r, out_off, src_off), want(H, W, "random", r), (H, W, r, out_off, src_off))


def test_argument_errors_launch_nothing(mbavo, gpu_ctx):
    import torch
    src = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    out = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda:0")
    for H, W, r in ((8, 8, 0), (8, 8, 4), (2, 8, 1), (8, 2, 1)):
        assert gpu_ctx.lib.mbavo_corner_score_u8(src.data_ptr(), H, W, r, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()
