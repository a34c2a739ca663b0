"""Caller-supplied masks (mbavo_pairs_opts.mask, mbavo_pairs_set_masks, mbavo_undistort_mask_batch, mbavo_mask_clearance_batch):
what can be held without a GPU.  The entries exist in the library, the header and the binding; mbavo_pairs_opts has not grown and
`mask` is its last word; mbavo_pairs_plan counts the stored masks and the pyramids of a mask = 1 object and nothing with mask = 0;
the options and the entries reject what include/mbavo.h says they reject; the two numpy forms of the warp
(tests/pairs_mask_ref.py) agree; a tap of weight 0 is not read; and the bonnet mask leaves the GPU tests something to drop and
something to keep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_api_support as api
import pairs_mask_ref as mref
import pairs_valid_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbavo_undistort_mask_batch", "mbavo_mask_clearance_batch", "mbavo_pairs_set_masks"]
SHAPES = [dict(), dict(B=3, L=3, H=50, W=70, cell=6), dict(B=64, H=480, W=640, fmt=2), dict(B=2, L=8, H=1024, W=1280, cell=40)]


def _align(v, a=256):
    return (v + a - 1) // a * a


def test_entry_points_are_exported_declared_and_listed(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbavo.h")).read(), flags=re.S)
    raw = C.CDLL(mbavo.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS, name
    assert re.search(r"\bint\s+mask\s*;", header) and re.search(r"\breserved2\s*\[\s*1\s*\]\s*;", header)
    assert lib.mbavo_abi_version() == 3


def test_the_options_struct_has_not_grown(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    P = capi.PairsOpts
    assert lib.mbavo_pairs_opts_size() == C.sizeof(P) == 272
    assert P.mask.offset == 268 == P.valid_radius.offset + 4 and P.mask.size == 4
    assert P.reserved.offset == 244 and P.reserved.size == 28  # `reserved` stays the name of the whole tail
    o = P()
    assert o.mask == 0  # a zeroed struct is today's behaviour
    o.mask = 1
    assert bytes(o)[268:272] == np.array([1], np.int32).tobytes() and list(o.reserved)[6] == 1 and list(o.reserved)[5] == 0
    o.reserved[6] = 0
    assert o.mask == 0


def test_a_zeroed_mask_field_is_the_plan_of_today(mbavo):
    """mask = 0: every rule and every byte as before -- r > 0 still needs undistort != 0, and the byte counts are those the
    clearance tests state (nothing with r = 0, one pyramid per map with r > 0)."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for kw in SHAPES:
        B, L, H, W = kw.get("B", 4), kw.get("L", 4), kw.get("H", 120), kw.get("W", 160)
        pyramid = sum(_align((H >> l) * (W >> l)) for l in range(L))
        for u in (0, 1, 2):
            o = api.opts(capi, keep=keep, **kw)
            o.undistort = u
            assert o.mask == 0
            base = api.plan(lib, o)
            assert base[0] == 0
            o.valid_radius = 2
            rc, nbytes, _ = api.plan(lib, o)
            assert (rc, nbytes) == ((api.E_ARG, -7) if u == 0 else (0, base[1] + pyramid)), (kw, u)


@pytest.mark.parametrize("kw", SHAPES)
def test_plan_counts_the_stored_masks_and_the_pyramids(mbavo, kw):
    """mask = 1 against the same options with mask = 0 (undistort = 0 with r > 0, which mask = 0 rejects: against r = 0): exactly G' x
    aligned(H W) bytes of stored masks more, and G' pyramids more where the mask = 0 object holds none -- r = 0, or undistort = 0;
    G' = max(num_cameras, 1).  The capacities do not move."""
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    B, L, H, W = kw.get("B", 4), kw.get("L", 4), kw.get("H", 120), kw.get("W", 160)
    pyramid = sum(_align((H >> l) * (W >> l)) for l in range(L))
    for u in (0, 1, 2):
        for G in (0, 1, 2, B):
            for r in (0, 1, 64):
                o = api.opts(capi, keep=keep, **kw)
                o.undistort, o.num_cameras = u, G
                had_pyramids = u != 0 and r > 0
                o.valid_radius = r if had_pyramids else 0
                base = api.plan(lib, o)
                assert base[0] == 0
                o.valid_radius, o.mask = r, 1
                rc, nbytes, cells = api.plan(lib, o)
                assert rc == 0 and cells == base[2], (u, G, r)
                want = max(G, 1) * (_align(H * W) + (0 if had_pyramids else pyramid))
                assert nbytes - base[1] == want, (u, G, r, nbytes - base[1], want)


def test_plan_rejects_a_bad_mask_field_and_a_bad_radius(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    keep = []
    for u, r, mask, ok in ((0, 0, 2, False), (1, 0, -1, False), (1, 1, 2, False), (2, 1, 1 << 30, False), (0, 0, -(1 << 31), False),
                           (0, 1, 0, False), (0, 64, 0, False),                       # mask = 0: r > 0 still needs undistort != 0
                           (0, -1, 1, False), (0, 65, 1, False), (1, 65, 1, False), (2, -1, 1, False),
                           (0, 0, 1, True), (0, 1, 1, True), (0, 64, 1, True), (1, 0, 1, True), (1, 64, 1, True), (2, 0, 1, True), (2, 2, 1, True),
                           (0, 0, 0, True), (1, 1, 0, True)):
        o = api.opts(capi, keep=keep)
        o.undistort, o.valid_radius, o.mask = u, r, mask
        rc, nbytes, _ = api.plan(lib, o)
        assert (rc == 0) == ok and (ok or (rc == api.E_ARG and nbytes == -7)), (u, r, mask, rc)


def test_the_entries_return_e_arg_before_they_touch_a_device(mbavo):
    lib = mbavo.load()
    assert lib.mbavo_undistort_mask_batch(None, 1, None, 60, 80, None, 50, 70, None) == api.E_ARG
    assert lib.mbavo_mask_clearance_batch(None, 1, None, None, 50, 70, 60, 80, 3, 1, None) == api.E_ARG
    assert lib.mbavo_pairs_set_masks(None, 0, 1, None) == api.E_ARG


# ---- the numpy restatement
def _maps():
    hand, _ = vref.handcrafted_map()
    return dict({n: vref.camera_map(c) for n, c in vref.CAMERAS.items()}, handcrafted=hand)


@pytest.mark.parametrize("mask", sorted(mref.MASKS))
def test_the_two_numpy_forms_of_the_warp_agree(mask):
    raw = mref.MASKS[mask]()
    assert raw.shape == (vref.HS, vref.WS) and raw.dtype == np.uint8 and (raw == 0).any() and (raw != 0).any()
    for name, m in _maps().items():
        loops, vec = mref.warp_mask_loops(raw, m), mref.warp_mask(raw, m)
        assert loops.dtype == vec.dtype == np.uint8 and loops.shape == (vref.H, vref.W)
        assert np.array_equal(loops, vec), (mask, name, int((loops != vec).sum()))
        assert set(np.unique(vec)) <= {0, 1}
        assert not vec[~vref.valid0(m, vref.HS, vref.WS)].any()  # an invalid entry is masked out whatever the mask says
    ones = np.full((vref.HS, vref.WS), 9, np.uint8)
    for name, m in _maps().items():  # a mask without a hole: the warp is the map term
        assert np.array_equal(mref.warp_mask(ones, m).astype(bool), vref.valid0(m, vref.HS, vref.WS)), name


def test_valid0_with_a_mask_is_the_and_of_both_terms():
    m = vref.camera_map(vref.CAMERAS["radtan"])
    mask = mref.bonnet_undistorted()
    both, only_map, only_mask = mref.valid0(m, mask), mref.valid0(m, None), mref.valid0(None, mask)
    assert np.array_equal(only_map, vref.valid0(m, vref.HS, vref.WS)) and np.array_equal(only_mask, mask != 0)
    assert np.array_equal(both, only_map & only_mask) and both.sum() < min(only_map.sum(), only_mask.sum())
    for r in (0, 1, 3):
        for a, b in zip(mref.clearance(m, mask, vref.L, r), vref.clearance(both, vref.L, r)):
            assert np.array_equal(a, b)
    for a, b in zip(mref.clearance(None, np.ones((vref.H, vref.W), np.uint8), vref.L, 2), vref.clearance(np.ones((vref.H, vref.W), bool), vref.L, 2)):
        assert np.array_equal(a, b) and not a[:2].any() and a[2:-2, 2:-2].all()  # no map, no hole: the rectangular border r


def test_a_tap_of_weight_zero_is_not_read():
    """On the handcrafted map the plain entries point at the whole coordinate (Ws / 2, Hs / 2): with its right, lower and diagonal
    neighbours masked the warped byte stays 1; the same entry moved by one nextafter towards them gives a tap of theirs a weight
    and becomes 0; moved the other way it reads (x0 - 1, y0) and (x0, y0), both usable, and stays 1."""
    hand, want = vref.handcrafted_map()
    raw = mref.planted()
    cx, cy = vref.WS // 2, vref.HS // 2
    assert raw[cy, cx] != 0 and raw[cy, cx + 1] == 0 and raw[cy + 1, cx] == 0 and raw[cy + 1, cx + 1] == 0
    assert raw[cy, cx - 1] != 0 and raw[cy - 1, cx] != 0
    r, c = 20, 33
    assert (r, c) not in want and tuple(hand[r, c]) == (np.float32(cx), np.float32(cy))
    inf = np.float32(np.inf)
    for warp in (mref.warp_mask_loops, mref.warp_mask):
        assert warp(raw, hand)[r, c] == 1
        for axis in (0, 1):
            m = hand.copy()
            m[r, c, axis] = np.nextafter(hand[r, c, axis], inf)
            assert warp(raw, m)[r, c] == 0, axis
            m[r, c, axis] = np.nextafter(hand[r, c, axis], -inf)
            assert warp(raw, m)[r, c] == 1, axis
    # the limit entries: (Ws - 1, Hs - 1) and (0, 0) read one tap each; the masked neighbours of (0, 0) do not reach it
    w = mref.warp_mask(raw, hand)
    for (rr, cc), ok in want.items():
        if not ok:
            assert w[rr, cc] == 0
    at = lambda x, y: tuple(np.argwhere((hand[..., 0] == np.float32(x)) & (hand[..., 1] == np.float32(y)))[0])
    assert w[at(vref.WS - 1, vref.HS - 1)] == 1
    zero = np.argwhere((hand[..., 0] == 0) & (hand[..., 1] == 0))  # 0.0 and -0.0: both entries
    assert len(zero) == 2 and all(w[tuple(z)] == 1 for z in zero)
    # an entry just inside a limit reaches the raw pixel next to the limit with a tiny weight: masked there, it is 0
    down = np.argwhere(hand[..., 0] == np.nextafter(np.float32(vref.WS - 1), -inf))
    assert len(down) == 1 and raw[1, vref.WS - 2] == 0 and raw[1, vref.WS - 1] != 0 and w[tuple(down[0])] == 0


@pytest.mark.parametrize("camera", sorted(vref.CAMERAS))
def test_input_condition_of_the_gpu_tests(camera):
    """At 50 x 70 with r = 1 the bonnet mask drops at least 10 % of the level-0 pixels that the clearance mask alone keeps, and keeps
    at least 25 % of them: the GPU tests have keypoints to drop and keypoints to keep."""
    r = 1
    m = vref.camera_map(vref.CAMERAS[camera])
    alone = vref.clearance(vref.valid0(m, vref.HS, vref.WS), vref.L, r)[0]
    masked = mref.clearance(m, mref.warp_mask(mref.bonnet(), m), vref.L, r)[0]
    assert not (masked & ~alone).any()
    kept = masked.sum() / alone.sum()
    print("bonnet, %s: keeps %.4f and drops %.4f of the %d clear level-0 pixels" % (camera, kept, 1.0 - kept, alone.sum()))
    assert 1.0 - kept >= 0.10 and kept >= 0.25


def test_input_condition_of_the_gpu_tests_without_a_map():
    """The same for the objects with undistort = 0: the bonnet drawn in the 50 x 70 image against the rectangular border r = 1."""
    r = 1
    alone = vref.clearance(np.ones((vref.H, vref.W), bool), vref.L, r)[0]
    masked = mref.clearance(None, mref.bonnet_undistorted(), vref.L, r)[0]
    kept = masked.sum() / alone.sum()
    print("bonnet, no map: keeps %.4f and drops %.4f" % (kept, 1.0 - kept))
    assert 1.0 - kept >= 0.10 and kept >= 0.25
