"""mbavo_pairs_match_brightness on the device, through the C ABI, against the numpy restatement (tests/pairs_photo_ref.py) run on
entries rebuilt on the host from the object's own device arrays (pairs_oracle.read_entry).

Shapes: B = 3 pairs of 48 x 64 textures at L = 3, grid cells of 8, border 1; the blurred frame of pair b is a shifted, noised copy
of its keyframe as a camera with gain and offset EXPOSURE[b] would have taken it.  Cases: k = 2 and k = 4; S = 3 (an odd remainder
of the two samples in flight) and S = 4; P = 1 and P = 8; the three keyframe formats; an every-candidate object at 96 x 128 with P =
8 (G = 64 workgroups, each serving more than one tile); the caller's points on two cameras under undistort = 1; a pair without
keypoints and a pair with a constant keyframe (degenerate); a pair moved off its knots (MBAVO_E_RANGE); the rendered pairs of
tests/golden/filter_scene.npz for the end-to-end property.

Bound.  status, num_keypoints, num_full and num_pixels are identical.  gain, cost_before, cost_after: |device - restatement| /
|restatement|; offset: |device - restatement| / max(|restatement|, 1 grey level) (an offset may be zero).  BOUND = 16 x the largest
such figure MEASURED over these cases on an MI355X (profiles/r42_pairs_photo.txt).  It is a measured number: the device's tap
and pose forms may differ from numpy's by a few ulps, but on every case here all four doubles came back equal to the restatement's
(the float32 blends of 8-bit taps absorb the last bits of a tap coordinate), so 16 x 0 asks for equality.  Every figure is printed before it is asserted (-s).
The correction is held bit for bit: to the restated correction with the DEVICE's (a, b), and to a twin object updated with it."""
import ctypes as C

import numpy as np
import pytest

import pairs_device as dv
import pairs_filter_scene as fs
import pairs_oracle as po
import pairs_photo_ref as pref
import pairs_photo_support as pp
import pairs_refine_scene as sc
from pairs_photo_support import B, CELL, EXPOSURE, H, L, THR, W  # noqa: F401  (the plain shape)
from pairs_photo_support import apply as _apply, images as _images, motion as _motion, prepared as _prepared, same_state as _same_state, state as _state

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, DEGENERATE = -1, -2, 1
MEASURED = 0.0  # the largest relative difference seen over these cases on an MI355X (profiles/r42_pairs_photo.txt): none at all
BOUND = 16 * MEASURED  # (so the doubles are asked to be the restatement's own)
PAT1 = np.array([[0, 0]], np.int32)
# (k, N, segment the samples lie on, S, pattern (None: the 8-pixel one), keyframe_format)
CASES = [(4, 4, 0, 3, None, 0), (2, 2, 0, 4, PAT1, 1), (4, 6, 1, 4, None, 2), (2, 2, 0, 3, None, 2)]
def _check(mbavo, ctx, pb, counts, k, tag, level=0, **kw):
    """pairs_photo_support.check under this file's bound."""
    return pp.check(mbavo, ctx, pb, counts, k, tag, level=level, bound=BOUND, **kw)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_against_restatement(mbavo, gpu_ctx, case):
    k = CASES[case][0]
    pb, counts = _prepared(gpu_ctx, CASES[case])
    try:
        assert (counts > 0).all()
        # (min_pixels = 8: a level with 12 keypoints, or 48 one-pixel patches, has fewer than the default's 64 pixels)
        _, w0 = _check(mbavo, gpu_ctx, pb, counts, k, "case %d level 0" % case, level=0, min_pixels=8)
        _, w1 = _check(mbavo, gpu_ctx, pb, counts, k, "case %d level %d, one round" % (case, L - 1), level=L - 1, rounds=1, min_pixels=8)
        _, w2 = _check(mbavo, gpu_ctx, pb, counts, k, "case %d level 1, defaults" % case, level=1)
        print("case %d: largest relative difference %.3g (bound %.3g)" % (case, max(w0, w1, w2), BOUND))
        out = _apply(pb, counts, "case %d apply" % case, level=0, rounds=2, min_pixels=8)
        assert any(r.status == 0 for r in out)
        # a second call fits what is left, on the corrected frame
        _check(mbavo, gpu_ctx, pb, counts, k, "case %d again" % case, level=0, min_pixels=8)
    finally:
        pb.close()


def test_correction_equals_an_update_with_the_corrected_frames(mbavo, gpu_ctx):
    pb, counts = _prepared(gpu_ctx, CASES[0])
    twin, counts2 = _prepared(gpu_ctx, CASES[0])
    try:
        assert np.array_equal(counts, counts2)
        out = _apply(pb, counts, "twin", level=1)
        c = _images()
        fixed = np.stack([pref.correct(c["blur"][b], out[b].gain, out[b].offset) if out[b].status == 0 else c["blur"][b] for b in range(B)])
        twin.update(dv.dev(np.ascontiguousarray(fixed))[0])
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(twin, counts), "twin")
    finally:
        pb.close()
        twin.close()


def test_same_bits_on_repeat_and_for_any_batch(mbavo, gpu_ctx):
    pb, counts = _prepared(gpu_ctx, CASES[0])
    try:
        rc1, out1 = pb.match_brightness(level=0)
        rc2, out2 = pb.match_brightness(level=0)
        assert rc1 == 0 and rc2 == 0 and bytes(out1) == bytes(out2)
        assert pb.match_brightness(level=0, want_records=False) == (0, None) and pb.photo_stats() == (4, 0, 0)
        for b in range(B):
            one, _ = _prepared(gpu_ctx, CASES[0], sel=slice(b, b + 1))
            try:
                rcb, outb = one.match_brightness(level=0)
                assert rcb == 0 and bytes(outb) == bytes(out1)[b * 48:(b + 1) * 48], b
            finally:
                one.close()
    finally:
        pb.close()


def test_every_candidate_tiles_shared_by_all_groups(mbavo, gpu_ctx):
    """96 x 128, every candidate, P = 8: tiles of 128 keypoints, G = 64 workgroups, K > 64 x 128 so that a workgroup serves more
    than one tile and the sums meet in workgroup order."""
    case = (2, 2, 0, 3, None, 0)
    pb, counts = _prepared(gpu_ctx, case, dense=True, h=96, w=128, levels=2, thr=0.5)
    try:
        print("every candidate: level-0 counts", counts[:, 0])
        assert counts[:, 0].min() > 64 * 128
        _check(mbavo, gpu_ctx, pb, counts, case[0], "every candidate", level=0, rounds=2)
        _apply(pb, counts, "every candidate apply", level=0, rounds=1)
    finally:
        pb.close()


def test_two_cameras_under_undistort(mbavo, gpu_ctx):
    """Object D of tests/pairs_oracle.py (the caller's points, undistort = 1, L = 3, S = 5, packed keyframe) on its first two cameras.
    The description is known to pairs_oracle under a name of its own for the length of this test only."""
    o = dict(po.OBJECTS["D"], cams=po.OBJECTS["D"]["cams"][:2], cam_of=(0, 1, 0))
    po.OBJECTS["D on two cameras"] = o
    try:
        pb, counts = po.make_object(gpu_ctx, "D on two cameras")
    finally:
        del po.OBJECTS["D on two cameras"]
    try:
        assert (counts[:, 0] > 8).all()
        _check(mbavo, gpu_ctx, pb, counts, o["k"], "two cameras", level=0, min_pixels=8)
        _check(mbavo, gpu_ctx, pb, counts, o["k"], "two cameras level 2", level=2, min_pixels=8, rounds=1)
        _apply(pb, counts, "two cameras apply", level=0, min_pixels=8)
    finally:
        pb.close()


def test_degenerate_pairs_are_left_alone(mbavo, gpu_ctx):
    """Pair 1 has no depth anywhere (K = 0); pair 2's keyframe is constant (the caller's points keep it its keypoints)."""
    case = CASES[0]
    c = _images()
    depth = c["depth"].copy()
    depth[1] = 0.0
    pb, counts = _prepared(gpu_ctx, case, depth=depth)
    try:
        assert (counts[1] == 0).all() and (counts[0] > 0).all()
        out, _ = _check(mbavo, gpu_ctx, pb, counts, case[0], "no depth", level=0)
        assert (out[1].status, out[1].num_full, out[1].cost_before, out[1].cost_after) == (DEGENERATE, 0, 0.0, 0.0) and out[0].status == 0
        out = _apply(pb, counts, "no depth apply", level=0)
        assert out[1].status == DEGENERATE
    finally:
        pb.close()
    rng = np.random.default_rng(5)
    sharp = c["sharp"].copy()
    sharp[2] = 100
    pts = [(rng.integers(8, 40, (12, 2)).astype(np.float64), rng.uniform(1.0, 3.0, 12)) for _ in range(B)]
    pb, counts = _prepared(gpu_ctx, case, sharp=sharp, points=pts)
    try:
        assert (counts[:, 0] == 12).all()
        out, _ = _check(mbavo, gpu_ctx, pb, counts, case[0], "constant keyframe", level=0)
        assert out[2].status == DEGENERATE and out[2].num_full > 8 and out[0].status == 0
        out = _apply(pb, counts, "constant keyframe apply", level=0)
        assert out[2].status == DEGENERATE
    finally:
        pb.close()


def test_pair_off_its_knots(mbavo, gpu_ctx):
    """mbavo_pairs_set_states can put a pair's times off its knots: that pair reports MBAVO_E_RANGE and nothing of it is changed."""
    case = CASES[3]
    pb, counts = _prepared(gpu_ctx, case)
    try:
        rc, good = pb.match_brightness(level=0)
        assert rc == 0
        m = _motion(case[0], case[1], case[2])
        states = (mbavo.capi.VoState * B)()
        for b, st in enumerate(states):  # the same knots and times through the state; pair 1's knots start long after its frame
            st.t0, st.dt, st.N, st.is_first = (100.0 if b == 1 else float(m["t0"][b])), m["dt"], case[1], 0
            st.knots_t[:3 * case[1]] = list(m["kt"][b].ravel())
            st.knots_R[:4 * case[1]] = list(m["kR"][b].ravel())
            st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
        assert pb.set_states(states) == 0
        out, _ = _check(mbavo, gpu_ctx, pb, counts, case[0], "off knots", level=0)
        assert (out[1].status, out[1].num_keypoints, out[1].num_full, out[1].num_pixels) == (E_RANGE, counts[1, 0], 0, 0)
        out = _apply(pb, counts, "off knots apply", level=0)
        assert out[1].status == E_RANGE
        for b in (0, 2):
            assert bytes(out[b]) == bytes(good[b])
    finally:
        pb.close()


def test_rejected_calls_launch_nothing(mbavo, gpu_ctx):
    from mba_vo_amd import workloads
    capi, lib = mbavo.capi, gpu_ctx.lib
    case = CASES[0]
    k, N, start, S, pattern, fmt = case
    c = _images()
    fresh = workloads.PairBatch(gpu_ctx, B, L=L, H=H, W=W, S=S, k=k, N=N, cell=CELL, thresh=THR, border=1, keyframe_format=fmt)
    try:
        out = (capi.PairsPhoto * B)()
        ok = pref.opts_struct(capi)
        assert pref.call(lib, fresh.handle, ok, out) == E_ARG  # before the first prepare
        fresh.prepare(*dv.dev(c["sharp"], c["depth"], c["blur"]))
        assert pref.call(lib, fresh.handle, ok, out) == E_ARG  # before the first motion
        assert fresh.photo_stats() == (0, 0, 0)
    finally:
        fresh.close()
    pb, counts = _prepared(gpu_ctx, case)
    try:
        before = _state(pb, counts)
        out = (capi.PairsPhoto * B)()
        assert pb.match_brightness(level=0)[0] == 0 and pb.photo_stats() == (4, 1, B * 48)
        nan, inf = float("nan"), float("inf")
        bad = [None, pref.opts_struct(capi, level=-1), pref.opts_struct(capi, level=L), pref.opts_struct(capi, rounds=-1), pref.opts_struct(capi, rounds=9),
               pref.opts_struct(capi, apply=2), pref.opts_struct(capi, apply=-1), pref.opts_struct(capi, min_pixels=-1), pref.opts_struct(capi, huber=-1.0),
               pref.opts_struct(capi, huber=nan), pref.opts_struct(capi, min_var=-1.0), pref.opts_struct(capi, min_var=inf),
               pref.opts_struct(capi, gain_min=-0.5), pref.opts_struct(capi, gain_min=nan), pref.opts_struct(capi, gain_max=inf),
               pref.opts_struct(capi, gain_max=-2.0), pref.opts_struct(capi, gain_min=2.0, gain_max=1.0), pref.opts_struct(capi, gain_min=5.0),
               pref.opts_struct(capi, gain_max=0.1)]
        for o in bad:
            assert pref.call(lib, pb.handle, o, out) == E_ARG and pb.photo_stats() == (0, 0, 0), None if o is None else bytes(o)
        assert lib.mbavo_pairs_match_brightness(None, C.byref(ok), out) == E_ARG
        _same_state(before, _state(pb, counts), "rejected")
        assert pb.match_brightness(level=1, rounds=8, want_records=False) == (0, None) and pb.photo_stats() == (9, 0, 0)
        assert pb.match_brightness(level=0, rounds=1, apply=True, want_records=False) == (0, None) and pb.photo_stats() == (2 + 1 + 1, 0, 0)
    finally:
        pb.close()
    # the stage's LDS limit: a level with more pattern pixels than a tile has items
    big = np.stack([np.arange(1025) % 5 - 2, np.arange(1025) // 205 - 2], 1).astype(np.int32)
    pb, counts = _prepared(gpu_ctx, (k, N, start, S, big, fmt))
    try:
        assert pref.call(lib, pb.handle, pref.opts_struct(capi), None) == E_ARG and pb.photo_stats() == (0, 0, 0)
    finally:
        pb.close()
    # ... or with so many blur samples that their pose entries do not fit beside the item arrays
    pb, counts = _prepared(gpu_ctx, (k, N, start, 300, pattern, fmt))
    try:
        assert pref.call(lib, pb.handle, pref.opts_struct(capi), None) == E_ARG and pb.photo_stats() == (0, 0, 0)
    finally:
        pb.close()


def test_matched_brightness_lets_the_lm_end_lower(mbavo, gpu_ctx):
    """The rendered pairs of tests/golden/filter_scene.npz, their blurred frames as a camera with gain 1.3 and offset -20 took
    them, the true knots moved by 3 cm as the start (through mbavo_pairs_set_motion: the fixture's k = 4 knots keep their own time
    base, which a predict would replace by the frame's): match_brightness(apply = 1) and then mbavo_lm_batch_levels ends at a lower
    level-0 report cost than the LM alone, on every pair.  The pose errors of both runs are printed, not asserted."""
    from mba_vo_amd import workloads
    capi = mbavo.capi
    c, m = sc.scene(), sc.motion()
    blur = np.stack([pref.exposed(fs.frames(b, noise=0.0)[0], 1.3, -20.0) for b in range(sc.B)])
    ends = {}
    for matched in (False, True):
        pb = workloads.PairBatch(gpu_ctx, sc.B, L=2, H=sc.H, W=sc.W, S=sc.S, k=sc.K_DEG, N=sc.N, cell=CELL, thresh=THR, border=4, huber=sc.HUBER)
        try:
            counts = pb.prepare(*dv.dev(np.ascontiguousarray(c["sharp"]), np.ascontiguousarray(c["depth"]), np.ascontiguousarray(blur)))
            assert (counts > 0).all() and pb.set_motion(m["cap"], m["exp"], m["t0"], m["dt"], m["kt"] + 0.03, m["kR"]) == 0
            if matched:
                rc, out = pb.match_brightness(level=1, apply=True)
                assert rc == 0 and all(r.status == 0 for r in out)
                print("matched:", [(round(r.gain, 4), round(r.offset, 3), round(r.cost_before, 1), round(r.cost_after, 1)) for r in out])
            dv.run_lm(gpu_ctx, capi, sc.B, 2, pb.array, sc.K_DEG)
            rep = pb.report(3.0)
            kt, kR = pb.knots()
            ends[matched] = ([r.cost for r in rep], [float(np.abs(kt[b] - m["kt"][b]).max()) for b in range(sc.B)],
                             [float(np.abs(kR[b] - m["kR"][b]).max()) for b in range(sc.B)])
            print("matched" if matched else "alone", "report status", [r.status for r in rep], "cost", [r.cost for r in rep])
            assert all(r.status == 0 for r in rep)
        finally:
            pb.close()
    for matched in (False, True):
        print("%s: level-0 report cost %s  largest knot error: translation %s  quaternion %s"
              % ("LM after match_brightness" if matched else "LM alone", ends[matched][0], ends[matched][1], ends[matched][2]))
    assert all(a < b_ for a, b_ in zip(ends[True][0], ends[False][0]))
