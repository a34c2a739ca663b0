"""Depth formats of mbavo_pairs (mbavo_pairs_opts.depth_format: 1 = ray distance, 2 = uint16 / depth_unit) and mbavo_depth_to_z.

Two routes to the same keypoints: the fused one (a prepare / update / track_frame that reads the raw maps and converts the pixels
it looks up) and the per-image one (mbavo_depth_to_z over every map, then a format-0 object on the result).  mbavo_depth_to_z is
held bit for bit to the numpy restatement of include/mbavo.h's formulas (tests/pairs_depth_ref.py); the fused route is held bit
for bit to the per-image one, in every count and keypoint array, for grid selection and every_candidate = 1, after a prepare and
after an update whose key list [0, 2] makes the place in the list differ from the pair index; launches, synchronisations and D2H
bytes are those of format 0; mbavo_lm_batch_levels cannot tell the two objects apart.

Shapes: 75 x 101 with L = 2 (odd sizes, rows that are no multiple of 64 or 256) and 96 x 128 with L = 3, B = 3; the larger one
also with B = 1 and B = 7.  The maps have holes (0, a value below 1e-2, a distance beyond depth_max) and, at positions the grid
selection looks up, the edge values of tests/test_pairs_depth_api.py."""
import ctypes as C

import numpy as np
import pytest

import lm_support as lms
import pairs_cases as cases
import pairs_dense_ref as dref
import pairs_depth_ref as zref
import pairs_device as dv
import pairs_ref
import pairs_step as ps
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

CELL, THR, E_ARG = 12, 3.0, -1
SHAPES = {"small": (75, 101, 2, 3, (90.0, 90.0, 50.0, 37.0)), "large": (96, 128, 3, 7, (110.0, 105.0, 63.5, 47.25))}
FORMATS = {0: dict(depth_format=0, depth_unit=0.0, depth_max=0.0), 1: zref.UNREAL, 2: zref.ETH3D}
SENTINEL = -7.0


def _borders(L):
    return [max(4, 8 >> l) for l in range(L)]


def _raw_maps(fmt, sharp, L, intr, seed):
    """B maps in format fmt for the keyframes `sharp`, and the planted positions [(b, x, y)]."""
    B, H, W = sharp.shape
    raw = cases.raw_depth(fmt, B, H, W, seed, beyond=150.0 if fmt == 1 else None)  # (beyond depth_max = 100)
    fx, fy, cx, cy = intr
    m, planted = _borders(L)[0], []
    for b in range(B):
        pk = [p for p in pairs_ref.picks(pairs_ref.gradient_magnitude(sharp[b]), 0, H, W, CELL, CELL, THR)
              if p is not None and m <= p[0] < W - m and m <= p[1] < H - m]
        for j, (x, y) in enumerate(pk[1::2]):
            n = np.sqrt(((x - cx) / fx) ** 2 + ((y - cy) / fy) ** 2 + 1.0)
            at = np.float32(0.01 * n if fmt == 1 else 0.01)  # z next to 1e-2 on both sides
            f32 = [np.nextafter(at, np.float32(0)), at, np.nextafter(at, np.float32(1)), np.nextafter(np.nextafter(at, np.float32(1)), np.float32(1)),
                   np.float32(100), np.nextafter(np.float32(100), np.float32(200)), np.float32(0.0102), np.float32(0.0125)]
            raw[b, y, x] = (50, 51, 0, 65535, 49, 52)[j % 6] if fmt == 2 else f32[j % 8]
            planted.append((b, x, y))
    if fmt != 2:  # what the detectors never look up, for mbavo_depth_to_z: the corner, the principal point, the last pixel
        raw[:, 0, 0], raw[:, int(cy), int(cx)], raw[:, -1, -1] = 0.0125, 0.01, 100.0
    else:
        raw[:, 0, 0], raw[:, -1, -1] = 50, 65535
    return raw, planted


_CASES = {}


def _case(shape, fmt):
    """Images, raw maps and the numpy z of one (shape, format), made once: B pairs, and new keyframes for an update."""
    key = (shape, fmt)
    if key not in _CASES:
        H, W, L, B, intr = SHAPES[shape]
        sharp = np.stack([synth.texture_image(H, W, seed=7 + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        new_sharp = np.stack([synth.texture_image(H, W, seed=40 + 3 * b, octaves=(16, 8, 4)) for b in range(B)])
        other = synth.texture_image(H, W, seed=107, octaves=(16, 8, 4))
        blur = np.stack([np.roll(other, (3 * b + 1, 5 * b + 2), (0, 1)) for b in range(B)])
        o = FORMATS[fmt]
        raw, planted = _raw_maps(fmt, sharp, L, intr, seed=11 + fmt)
        new_raw, new_planted = _raw_maps(fmt, new_sharp, L, intr, seed=23 + fmt)
        z = zref.to_z(fmt, raw, intr, o["depth_unit"], o["depth_max"])
        new_z = zref.to_z(fmt, new_raw, intr, o["depth_unit"], o["depth_max"])
        for zz, pl in ((z, planted), (new_z, new_planted)):  # the planted values fall on both sides of the depth test
            kept = [bool(zref.has_depth(zz[b, y, x])) for b, x, y in pl if b < 3]
            assert len(kept) >= 12 and 3 <= sum(kept) <= len(kept) - 3, kept
        _CASES[key] = dict(H=H, W=W, L=L, B=B, intr=intr, opts=o, sharp=np.ascontiguousarray(sharp), blur=np.ascontiguousarray(blur), raw=raw, z=z,
                           new_sharp=np.ascontiguousarray(new_sharp), new_blur=np.ascontiguousarray(np.roll(blur, (2, 3), (1, 2))),
                           new_raw=new_raw, new_z=new_z)
    return _CASES[key]


def _batch(ctx, c, B, fmt, dense, **kw):
    from mba_vo_amd import workloads
    o = FORMATS[fmt]
    return workloads.PairBatch(ctx, B, L=c["L"], H=c["H"], W=c["W"], intr=c["intr"], border=_borders(c["L"]), cell=0 if dense else CELL, thresh=THR,
                               every_candidate=dense, **dict(o, **kw))


def _to_z(ctx, c, fmt, raw_t):
    from mba_vo_amd import workloads
    o = FORMATS[fmt]
    return workloads.depth_to_z(ctx, fmt, raw_t, c["intr"], o["depth_unit"], o["depth_max"])


def _assert_restatement(got, z_of_pair, c, dense, tag):
    """Every (pair, level) against numpy on the numpy z maps; (candidates dropped by the depth test, by the border test)."""
    H, W, L, borders = c["H"], c["W"], c["L"], _borders(c["L"])
    no_depth = no_border = 0
    for e, g in enumerate(got):
        b, l = divmod(e, L)
        im = g["ref"].reshape(H >> l, W >> l)
        if dense:
            rxy, rz = dref.keypoints(im, l, THR, z_of_pair[b], borders[l])
            full = int((pairs_ref.gradient_magnitude(im) > np.float32(THR)).sum())
            nob = len(dref.keypoints(im, l, THR, z_of_pair[b], 0)[1])
        else:
            rxy, rz = pairs_ref.keypoints(im, l, H, W, CELL, CELL, THR, z_of_pair[b], borders[l])
            full = sum(p is not None for p in pairs_ref.picks(pairs_ref.gradient_magnitude(im), l, H, W, CELL, CELL, THR))
            nob = len(pairs_ref.keypoints(im, l, H, W, CELL, CELL, THR, z_of_pair[b], 0)[1])
        assert dv.same_bits(g["xy"], rxy) and dv.same_bits(g["z"], rz), (tag, e)
        no_depth += full - nob
        no_border += nob - len(rz)
    return no_depth, no_border


@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("fmt", [1, 2])
def test_depth_to_z_matches_numpy_bit_for_bit(mbavo, gpu_ctx, shape, fmt):
    """Check 1: every pixel of every map, the last row and column included."""
    c = _case(shape, fmt)
    z = _to_z(gpu_ctx, c, fmt, dv.dev_depth(c["raw"])).cpu().numpy()
    assert z.dtype == np.float32 and dv.same_bits(z, c["z"])
    assert np.all(z[:, -1, -1] > 1) and np.all(z[:, -1, :].max(1) > 0) and (~zref.has_depth(z)).any() and zref.has_depth(z).any()
    one = _to_z(gpu_ctx, c, fmt, dv.dev_depth(c["raw"][1])).cpu().numpy()  # a single H x W map
    assert dv.same_bits(one, c["z"][1])


def test_depth_to_z_format_0_returns_its_input(mbavo, gpu_ctx):
    c = _case("small", 1)
    raw = c["raw"].copy()
    raw[0, 3, 5] = -0.0
    assert dv.same_bits(_to_z(gpu_ctx, c, 0, dv.dev_depth(raw)).cpu().numpy(), raw)


def test_depth_to_z_rejects_bad_arguments_without_a_launch(mbavo, gpu_ctx):
    """Check 6: a bad format or unit, a NULL pointer, H or W < 1: MBAVO_E_ARG and the output is not written."""
    import torch
    lib, c = gpu_ctx.lib, _case("small", 2)
    H, W = c["H"], c["W"]
    src = dv.dev_depth(c["raw"][0])
    out = torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda:0")
    K = (C.c_double * 4)(*c["intr"])
    call = lambda fmt, s, h, w, k, unit, o: lib.mbavo_depth_to_z(gpu_ctx.handle, fmt, s, h, w, k, unit, 0.0, o)
    s, o = src.data_ptr(), out.data_ptr()
    bad = [(3, s, H, W, K, 5000.0, o), (-1, s, H, W, K, 5000.0, o), (2, s, H, W, K, 0.0, o), (2, s, H, W, K, -5000.0, o), (2, None, H, W, K, 5000.0, o),
           (2, s, H, W, K, 5000.0, None), (1, s, H, W, None, 0.0, o), (2, s, 0, W, K, 5000.0, o), (2, s, H, 0, K, 5000.0, o), (1, s, -3, W, K, 0.0, o)]
    for args in bad:
        assert call(*args) == E_ARG, args[0:1] + args[2:4] + args[5:6]
    assert lib.mbavo_depth_to_z(None, 2, s, H, W, K, 5000.0, 0.0, o) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(2, s, H, W, K, 5000.0, o) == 0  # and the same call with good arguments writes it
    torch.cuda.synchronize()
    assert dv.same_bits(out.cpu().numpy(), c["z"][0])


_FUSED = {}  # (shape, fmt, dense) -> what the B = 3 fused prepare gave, for the runs with another B


@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_prepare_on_raw_maps_equals_format_0_on_converted_maps(mbavo, gpu_ctx, shape, fmt, dense):
    """Check 2, B = 3: every count and every array of every (pair, level) bit-identical between the two routes, and equal to
    numpy on the numpy z maps; the depth test and the border test each dropped something."""
    c = _case(shape, fmt)
    B = 3
    ts, tb = dv.dev(c["sharp"][:B], c["blur"][:B])
    raw_t = dv.dev_depth(c["raw"][:B])
    fused, twin = _batch(gpu_ctx, c, B, fmt, dense), _batch(gpu_ctx, c, B, 0, dense)
    try:
        cf = fused.prepare(ts, raw_t, tb)
        ct = twin.prepare(ts, _to_z(gpu_ctx, c, fmt, raw_t), tb)
        assert np.array_equal(cf, ct) and cf.min() > 0
        got = dv.read_batch(fused, cf)
        dv.assert_twins(got, dv.read_batch(twin, ct), (shape, fmt, dense))
        no_depth, no_border = _assert_restatement(got, c["z"], c, dense, (shape, fmt, dense))
        assert no_depth > 0 and no_border > 0
        assert fused.stats() == twin.stats()
        _FUSED[(shape, fmt, dense)] = got
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_a_pairs_results_do_not_depend_on_B(mbavo, gpu_ctx, fmt, dense):
    """96 x 128, L = 3 with B = 1 and B = 7: the pairs they share with the B = 3 run hold the same bits."""
    c = _case("large", fmt)
    L = c["L"]
    runs = {}
    if ("large", fmt, dense) in _FUSED:
        runs[3] = _FUSED[("large", fmt, dense)]
    for B in (1, 7) if 3 in runs else (1, 3, 7):
        pb = _batch(gpu_ctx, c, B, fmt, dense)
        try:
            counts = pb.prepare(*dv.dev(c["sharp"][:B]), dv.dev_depth(c["raw"][:B]), *dv.dev(c["blur"][:B]))
            runs[B] = dv.read_batch(pb, counts)
        finally:
            pb.close()
    dv.assert_twins(runs[1], runs[7][:L], ("B = 1 / 7", fmt, dense))
    dv.assert_twins(runs[3], runs[7][:3 * L], ("B = 3 / 7", fmt, dense))
    _assert_restatement(runs[7], c["z"], c, dense, ("B = 7", fmt, dense))
    assert not dv.same_bits(runs[7][0]["z"], runs[7][6 * L]["z"])


def _capacities(c, dense):
    return dref.capacities(c["H"], c["W"], c["L"]) if dense else pairs_ref.cells_per_level(c["H"], c["W"], c["L"], CELL, CELL)


@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("dense", [False, True])
def test_update_on_raw_maps_equals_format_0_on_converted_maps(mbavo, gpu_ctx, shape, fmt, dense):
    """Check 3: B = 3, new keyframes for the pairs [0, 2] -- map 1 of the two that are passed belongs to pair 2 -- whose maps
    differ from the old ones.  Both routes agree bit for bit, and with numpy on the composite maps; pair 1's keyframe arrays
    were filled with a sentinel before the update and hold it afterwards over their whole capacity."""
    c = _case(shape, fmt)
    B, L, keys = 3, c["L"], [0, 2]
    ts, tb = dv.dev(c["sharp"][:B], c["blur"][:B])
    raw_t = dv.dev_depth(c["raw"][:B])
    new_s, new_b = dv.dev(np.ascontiguousarray(c["new_sharp"][keys]), c["new_blur"][:B])
    new_raw_t = dv.dev_depth(np.ascontiguousarray(c["new_raw"][keys]))
    assert not np.array_equal(c["new_raw"][keys], c["raw"][keys])
    caps = _capacities(c, dense)
    fused, twin = _batch(gpu_ctx, c, B, fmt, dense), _batch(gpu_ctx, c, B, 0, dense)
    try:
        before = fused.prepare(ts, raw_t, tb)
        assert np.array_equal(twin.prepare(ts, _to_z(gpu_ctx, c, fmt, raw_t), tb), before)
        for pb in (fused, twin):
            for l in range(L):
                q = pb.array[1 * L + l]
                dv.poke(q.d_kp_xy, np.full(2 * caps[l], SENTINEL))
                dv.poke(q.d_kp_z, np.full(caps[l], SENTINEL))
                dv.poke(q.d_ref_dIxy, np.full(q.H * q.W * 8, 0xA5, np.uint8))
        cf = fused.update(new_b, keys, new_s, new_raw_t)
        ct = twin.update(new_b, keys, new_s, _to_z(gpu_ctx, c, fmt, new_raw_t))
        assert np.array_equal(cf, ct) and np.array_equal(cf[1], before[1]) and not np.array_equal(cf[keys], before[keys])
        assert fused.step_stats()[0] == twin.step_stats()[0]
        got, want = dv.read_batch(fused, cf), dv.read_batch(twin, ct)
        listed = [e for e in range(B * L) if e // L in keys]
        dv.assert_twins([got[e] for e in listed], [want[e] for e in listed], (shape, fmt, dense))
        z_now = c["z"][:B].copy()
        z_now[keys] = c["new_z"][keys]
        for b in keys:  # (level 0 of a listed pair is its new keyframe)
            assert np.array_equal(got[b * L]["ref"], c["new_sharp"][b].ravel())
        _assert_restatement([got[e] for e in listed], {0: z_now[0], 1: z_now[2]}, c, dense, ("update", shape, fmt, dense))
        for pb, arrays in ((fused, got), (twin, want)):
            for l in range(L):
                q = pb.array[1 * L + l]
                assert np.all(dv.peek(q.d_kp_xy, 2 * caps[l], np.float64) == SENTINEL) and np.all(dv.peek(q.d_kp_z, caps[l], np.float64) == SENTINEL), l
                assert np.all(arrays[L + l]["grad"] == 0xA5), l
                assert dv.same_bits(arrays[L + l]["cur"], want[L + l]["cur"])
    finally:
        fused.close()
        twin.close()


@pytest.mark.parametrize("dense", [False, True])
def test_launches_synchronisations_and_bytes_are_those_of_format_0(mbavo, gpu_ctx, dense):
    """Check 4: mbavo_pairs_last_stats after a prepare, mbavo_pairs_update_stats after an update and after a
    mbavo_pairs_track_frame (with mbavo_pairs_track_stats) are the same for formats 0, 1 and 2; and the frames a format-1 object
    tracks are, bit for bit, those of a format-0 object on the converted maps."""
    capi = mbavo.capi
    B, keys, k = 3, [0, 2], 2
    seen, frames = {}, {}
    for fmt in (0, 1, 2):
        c = _case("small", fmt or 1)
        ts, tb = dv.dev(c["sharp"][:B], c["blur"][:B])
        new_s, new_b = dv.dev(np.ascontiguousarray(c["new_sharp"][keys]), c["new_blur"][:B])
        raw_t, new_raw_t = dv.dev_depth(c["raw"][:B]), dv.dev_depth(np.ascontiguousarray(c["new_raw"][keys]))
        if fmt == 0:  # the format-1 maps, converted
            raw_t, new_raw_t = _to_z(gpu_ctx, c, 1, raw_t), _to_z(gpu_ctx, c, 1, new_raw_t)
        pb = _batch(gpu_ctx, c, B, fmt, dense, S=2, k=k, N=2, pattern=np.array([[0, 0]], np.int32))
        try:
            assert pb.stats()[:3] == (0, 0, 0)
            c0 = pb.prepare(ts, raw_t, tb)
            after_prepare = pb.stats()
            pb.update(new_b, keys, new_s, new_raw_t)
            after_update = pb.step_stats()[0]
            assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0
            out, counts, _, _ = pb.track_frame(tb, np.full(B, 0.1), np.full(B, 0.02), lms.lm_batch_opts(capi, k, 3), (ps.FLOW0, ps.FLOW1, ps.KERNEL), keys,
                                               dv.dev(np.ascontiguousarray(c["sharp"][keys]))[0], raw_t[0::2].contiguous())
            assert np.array_equal(counts, c0)  # the first keyframes again
            assert all(out[b].a.status == 0 and out[b].a.num_keypoints0 == counts[b, 0] for b in range(B))
            seen[fmt] = (after_prepare, after_update, pb.step_stats()[0], pb.track_stats())
            frames[fmt] = [bytes(out[b]) for b in range(B)]
        finally:
            pb.close()
    assert seen[0] == seen[1] == seen[2], seen
    assert seen[0][0][1] == 1 and seen[0][1][1] == 1 and seen[0][0][2] == 4 * B * 2
    assert frames[1] == frames[0]


def test_lm_cannot_tell_the_two_objects_apart(mbavo, gpu_ctx):
    """Check 5: B = 3, 96 x 128, L = 3: one mbavo_lm_batch_levels call on the format-2 object and on its format-0 twin: identical
    results, trace records and knots."""
    capi = mbavo.capi
    c = _case("large", 2)
    B, L, k, N = 3, c["L"], 2, 2
    ts = dv.dev(c["sharp"][:B])[0]
    tb = dv.dev(np.ascontiguousarray(np.roll(c["sharp"][:B], (1, 1), (1, 2))))[0]
    raw_t = dv.dev_depth(c["raw"][:B])
    kw = dict(S=4, k=k, N=N, pattern=np.array([[0, 0]], np.int32))
    fused, twin = _batch(gpu_ctx, c, B, 2, False, **kw), _batch(gpu_ctx, c, B, 0, False, **kw)
    try:
        cf = fused.prepare(ts, raw_t, tb)
        # every level of every pair hands the LM keypoints (the coarsest, 24 x 32 with a sixth of its depths missing, only a few);
        # that steps are taken on them is asserted below
        assert np.array_equal(twin.prepare(ts, _to_z(gpu_ctx, c, 2, raw_t), tb), cf) and cf.min() > 0
        rng = np.random.default_rng(2)
        kt0 = rng.normal(0, 2e-3, (B, N, 3))
        kR0 = np.tile(np.array([0.0, 0, 0, 1]), (B, N, 1)) + rng.normal(0, 1e-3, (B, N, 4))
        kR0 /= np.linalg.norm(kR0, axis=2, keepdims=True)
        motion = (np.full(B, 0.3), np.full(B, 0.04), np.zeros(B), 0.5, kt0, kR0)
        runs = []
        for pb in (fused, twin):
            assert pb.set_motion(*motion) == 0
            fields, recs, kinds = dv.run_lm(gpu_ctx, capi, B, L, pb.array, k)
            runs.append((fields, recs, pb.knots()))
            print("lm on %s: trace kinds %s, knots moved by %.3g" % ("fused" if pb is fused else "twin", sorted(kinds), np.abs(runs[-1][2][0] - kt0).max()))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
        assert dv.same_bits(runs[0][2][0], runs[1][2][0]) and dv.same_bits(runs[0][2][1], runs[1][2][1])
        assert sum(len(r) for r in runs[0][1]) > 0 and np.abs(runs[0][2][0] - kt0).max() > 1e-9  # steps were taken: not vacuous
    finally:
        fused.close()
        twin.close()
