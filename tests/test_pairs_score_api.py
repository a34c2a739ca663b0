"""mbavo_pairs_set_detector, mbavo_corner_score_u8 and their companions without a GPU: the entries exist in the library, the header
and the binding, the options have the size the header states, the ABI and mbavo_pairs_opts are what they were, NULL handles and
bad arguments are rejected before any device is touched -- and the numpy restatement of the score (tests/pairs_score_ref.py) has
the properties the definition states: the three exact zeros, integer sums that reach their maxima inside int with an exact double
argument, and the clamp.

d < 0 before the clamp: over 10^5 random windows (sums drawn as sums of n products of differences in -255 .. 255) the count is
printed (`-s`); it was 0 on the seed used here.  It can occur only through the rounding of the square root, where b = 0 or the
argument is a perfect square's neighbour; where it does, the clamp gives a score of exactly 0, which the test asserts on
constructed cases.
Every test here asks the library for the new entries first: none passes where mbavo_pairs_set_detector does not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_score_ref as sr

E_ARG = -1
NEW = ["mbavo_corner_score_u8", "mbavo_pairs_detector_opts_size", "mbavo_pairs_set_detector", "mbavo_pairs_detector_stats"]


@pytest.fixture(autouse=True)
def the_call_exists(mbavo):
    assert mbavo.load().mbavo_pairs_detector_opts_size() == C.sizeof(mbavo.capi.PairsDetectorOpts)


def test_entries_struct_size_abi_and_null_handles(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert "int %s(" % name in header
    assert "} mbavo_pairs_detector_opts;" in header
    assert lib.mbavo_pairs_detector_opts_size() == C.sizeof(capi.PairsDetectorOpts) == 32
    assert [n for n, _ in capi.PairsDetectorOpts._fields_] == ["score", "radius", "score_threshold", "reserved"]
    assert sum(C.sizeof(t) for _, t in capi.PairsDetectorOpts._fields_) == 32 and bytes(capi.PairsDetectorOpts()) == bytes(32)
    assert lib.mbavo_abi_version() == 3        # the change only adds
    assert lib.mbavo_pairs_opts_size() == 272  # the switch is a call, not a word of the options
    assert lib.mbavo_pairs_set_detector(None, C.byref(capi.PairsDetectorOpts())) == E_ARG
    assert lib.mbavo_pairs_set_detector(None, None) == E_ARG
    assert lib.mbavo_pairs_detector_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert mbavo.load().mbavo_pairs_detector_opts_size() == 32
    for name in ("set_detector", "detector_stats"):
        assert callable(getattr(workloads.PairBatch, name))


def test_set_detector_launches_copies_and_waits_for_nothing(mbavo):
    """The header's promise, on the call's own source: between its signature and the next function of pairs_score.hip there is no
    launch, no copy, no memset and no synchronisation (its one device call is the allocation of the first score = 1), so neither an
    accepted nor a rejected call can enqueue anything.  The launch statistics of the other calls cannot show this."""
    assert mbavo.load().mbavo_pairs_detector_opts_size() == 32
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "mba-vo_amd", "csrc", "pairs_score.hip")).read()
    first = src.index("int PairBatch::set_detector(")
    body = src[first:src.index("ScoreSlices PairBatch::score_slices()", first)]
    assert body.count("alloc(") == 1 and "return MBAVO_E_ARG" in body
    for word in ("hipLaunchKernelGGL", "<<<", "hipMemcpy", "hipMemset", "Synchronize", "score_levels", "refresh("):
        assert word not in body, word
    # every rejection comes before the allocation
    assert body.rindex("return MBAVO_E_ARG") < body.index("alloc(")


def test_corner_score_argument_errors_need_no_device(mbavo):
    """Checked before anything is launched: the pointers are never dereferenced."""
    lib = mbavo.load()
    src, dst = C.c_void_p(4096), C.c_void_p(8192)
    assert lib.mbavo_corner_score_u8(None, 8, 8, 1, dst, None) == E_ARG
    assert lib.mbavo_corner_score_u8(src, 8, 8, 1, None, None) == E_ARG
    for radius in (0, 4, -1):
        assert lib.mbavo_corner_score_u8(src, 8, 8, radius, dst, None) == E_ARG
    for H, W in ((2, 8), (8, 2), (0, 8), (8, -3)):
        assert lib.mbavo_corner_score_u8(src, H, W, 2, dst, None) == E_ARG


@pytest.mark.parametrize("r", [1, 2, 3])
def test_three_identities_are_exact_zeros(mbavo, r):
    H, W = 23, 31
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(5)
    assert not sr.score(np.full((H, W), 200, np.uint8), r).any()                             # a constant
    cols = rng.integers(0, 256, W).astype(np.uint8)
    img = np.broadcast_to(cols, (H, W)).copy()                                               # ky = 0 everywhere
    kx, ky = sr.differences(img)
    assert not ky.any() and kx.any() and not sr.score(img, r).any()
    assert not sr.score(np.where(x >= W // 2, 255, 0).astype(np.uint8), r).any()             # the vertical step edge
    diag = rng.integers(0, 256, H + W).astype(np.uint8)
    img = diag[x + y]                                                                        # I(x, y) = f(x + y): kx = ky inside
    kx, ky = sr.differences(img)
    assert np.array_equal(kx, ky) and kx.any() and not sr.score(img, r).any()
    assert sr.score(rng.integers(0, 256, (H, W)).astype(np.uint8), r).max() > 10             # (and it is not zero everywhere)


def test_sums_reach_their_maxima_inside_int_and_the_argument_is_exact(mbavo):
    r, top = 3, 49 * 255 * 255
    img = sr.checkerboard(24, 28)
    a, b, c = sr.sums(img, r)
    assert a.max() == top and c.max() == top and np.abs(b).max() <= top and 2 * top < 2 ** 31  # (a + c is formed in int too)
    assert a[12, 14] == top and c[12, 14] == top                                                # an interior window
    # the double argument against Python integers, on these sums and on the extreme corners of the range
    cases = [(int(a_), int(b_), int(c_)) for a_, b_, c_ in zip(a.ravel(), b.ravel(), c.ravel())]
    cases += [(top, top, 0), (top, -top, 0), (0, top, top), (top, 0, 0), (0, -top, 0)]
    for a_, b_, c_ in cases:
        exact = (a_ - c_) ** 2 + 4 * b_ * b_
        assert exact < 2 ** 53
        got = np.float64(a_ - c_) * np.float64(a_ - c_) + 4.0 * np.float64(b_) * np.float64(b_)
        assert int(got) == exact and float(got) == float(exact)
    # kx = ky with full contrast: b reaches the maximum as well, and the score is still an exact zero
    y, x = np.mgrid[0:24, 0:28]
    img = (255 * (((x + y) >> 1) & 1)).astype(np.uint8)
    a, b, c = sr.sums(img, r)
    assert a.max() == top and b.max() == top and c.max() == top and not sr.score(img, r).any()


def test_clamp_and_how_often_d_is_negative(mbavo):
    rng = np.random.default_rng(11)
    n_win, r = 100000, 3
    n = (2 * r + 1) ** 2
    kx, ky = rng.integers(-255, 256, (n_win, n)), rng.integers(-255, 256, (n_win, n))
    kx[: n_win // 4] = 0                       # a quarter each of the degenerate families, where d sits at the edge
    ky[n_win // 4: n_win // 2] = kx[n_win // 4: n_win // 2]
    a, b, c = (kx * kx).sum(1), (kx * ky).sum(1), (ky * ky).sum(1)
    sc, d = sr.score_of_sums(a, b, c, r, with_d=True)
    neg = int((d < 0).sum())
    print("d < 0 before the clamp in %d of %d windows (min d %.3g)" % (neg, n_win, d.min()))
    assert np.all(sc[d <= 0] == 0) and np.all(sc >= 0) and not np.isnan(sc).any()
    assert not sc[: n_win // 2].any()          # the two families are exact zeros whatever the window holds
    # constructed: a d below zero, had the square root rounded up, still scores 0
    s0, d0 = sr.score_of_sums(np.array([5]), np.array([0]), np.array([0]), 1, with_d=True)
    assert d0[0] == 0 and s0[0] == 0
    clamped = np.sqrt(np.where(np.array([-1e-9]) < 0, 0.0, np.array([-1e-9])) / 72.0).astype(np.float32)
    assert clamped[0] == 0


def test_restated_selection_swaps_the_response_only(mbavo):
    """The swapped host detector picks by score; outside the context the old response is back."""
    import pairs_ref
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (32, 40)).astype(np.uint8)
    depth = np.ones((32, 40), np.float32)
    before = pairs_ref.gradient_magnitude(img)
    xy1, _ = sr.keypoints(img, 0, 32, 40, 8, 4.0, depth, 2, 2, dense=False)
    assert np.array_equal(pairs_ref.gradient_magnitude(img), before)
    xy0, _ = sr.keypoints(img, 0, 32, 40, 8, 4.0, depth, 2, 0, dense=False)
    assert len(xy1) and len(xy0) and not np.array_equal(xy0, xy1)
    s = sr.score(img, 2)
    for x, y in xy1.astype(int):
        cy, cx = y // 8 * 8, x // 8 * 8
        assert s[y, x] == s[cy:cy + 8, cx:cx + 8].max() > 4.0
    xd, _ = sr.keypoints(img, 0, 32, 40, 8, 4.0, depth, 2, 2, dense=True)
    want = np.argwhere(s[2:-2, 2:-2] > np.float32(4.0))[:, ::-1] + 2
    assert np.array_equal(xd.astype(int), want)
