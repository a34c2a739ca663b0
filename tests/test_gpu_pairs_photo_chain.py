"""mbavo_pairs_match_brightness in chains with its neighbours: what the header promises about the calls behind an apply = 1.

Readers.  After apply = 1 on one object a twin takes pairs_photo_ref.correct of the same frames under the device's (a, b) through
mbavo_pairs_update.  The two objects then hold the same bytes (tests/test_gpu_pairs_photo.py asserts that much), and every reader --
mbavo_pairs_report, refine_depths, search_depths, filter_depths, the hypothesis pick, mbavo_lm_batch_levels -- returns the same
bytes on both.  The readers have also run on both objects BEFORE the correction, so a stage that kept anything derived from the old
current frame would answer differently on the object whose frame changed underneath it.  On object A of tests/pairs_oracle.py
(undistort = 0: a twin can be updated with host-corrected frames; packed keyframe, 75 x 101, start = 1) and on the plain B = 3,
48 x 64, L = 3 shape of tests/pairs_photo_support.py.

Lifetime.  The correction holds until the next frame: after apply = 1, a new frame through mbavo_pairs_update (n_key = 0) or
mbavo_pairs_track_frame leaves the object bit for bit what a twin holds that took the same frame and was never matched.

State.  On an object that has run filter_depths, carry_save and one track_frame, apply = 1 changes no byte of the filter state, the
tracker state or the hand-over state (pairs_photo_support.state, extended); on object B the masks select the same keypoints
afterwards as on an untouched object (pairs_photo_support.masks_probe).

After a prune (A, pairs_prune_support's keep patterns) and after a carry to the next keyframe (B, pair 2, as
tests/test_gpu_pairs_depth_options.py does it) a report-only call equals the restatement on pairs_oracle.read_entry of the object as it
now is: integers identical, doubles within 1e-9 (pairs_photo_support.BOUND: the project's figure behind the device's pose prologue).
Everything else here is bit for bit."""
import numpy as np
import pytest

import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po
import pairs_photo_ref as pref
import pairs_photo_support as pp
import pairs_prune_support as psup

pytestmark = pytest.mark.gpu

PLAIN = (4, 4, 0, 3, None, 0)      # (k, N, segment, S, pattern, keyframe_format) of tests/test_gpu_pairs_photo.py's first case
TRACKED = (2, 2, 0, 3, None, 0)    # N = 2: the tracker's initial states


def _counts_now(pb):
    return np.array([[pb.array[b * pb.L + l].K for l in range(pb.L)] for b in range(pb.B)], np.int32)


def _read(pb, k, ctx, capi, states=None, times=None):
    """Every reader once, as bytes: report, refine (report only), search, filter, the hypothesis pick (with states), the LM."""
    out = {}
    out["report"] = bytes(pb.report(3.0))
    rec, arr, _ = ds.refine_run(pb, level=-1)
    out["refine"] = bytes(rec) + b"".join(arr[key].tobytes() for key in sorted(arr))
    rec, arr = ds.search_run(pb, dc.ND, *dc.ABSOLUTE)
    out["search"] = bytes(rec) + b"".join(arr[key].tobytes() for key in sorted(arr))
    rc, rec = pb.filter_depths(level=-1, apply=False, **dc.FILTER)
    assert rc == 0
    st, _ = ds.filter_state(pb)
    out["filter"] = bytes(rec) + b"".join(st[key].tobytes() for key in ("mu", "info", "n_obs", "n_rej"))
    if states is not None:
        assert pb.set_states(states) == 0
        rc, rec = pb.predict_hypotheses(times[0], times[1], [0.0, 1.5], [None, (0.02, -0.01, 0.015, 0.004, -0.003, 0.002)], level=pb.L - 1)
        assert rc == 0
        out["hypotheses"] = bytes(rec) + b"".join(a.tobytes() for a in pb.knots())
    return out


def _lm(pb, k, ctx, capi):
    fields, recs, _ = dv.run_lm(ctx, capi, pb.B, pb.L, pb.array, k)
    return b"".join(fields) + b"".join(b"".join(r) for r in recs) + b"".join(a.tobytes() for a in pb.knots())


def _readers_agree(mbavo, ctx, make, blur, k, tag, level, states=None, times=None, **kw):
    """blur: the B x H x W frames both objects hold.  make() -> (pb, counts)."""
    capi = mbavo.capi
    pb, counts = make()
    twin, counts2 = make()
    try:
        assert np.array_equal(counts, counts2)
        first = _read(pb, k, ctx, capi), _read(twin, k, ctx, capi)  # (both on the uncorrected frames: whatever a stage keeps, it now has)
        assert first[0] == first[1], tag
        out = pp.apply(pb, counts, tag, level=level, extended=True, **kw)
        assert sum(r.status == 0 for r in out) >= 2
        fixed = np.stack([pref.correct(blur[b], out[b].gain, out[b].offset) if out[b].status == 0 else blur[b] for b in range(pb.B)])
        assert not np.array_equal(fixed, blur)
        twin.update(dv.dev(np.ascontiguousarray(fixed))[0])
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(twin, counts), tag)
        pp.same_state(pp.state(pb, counts, extended=True), pp.state(twin, counts, extended=True), tag)
        got, want = _read(pb, k, ctx, capi, states, times), _read(twin, k, ctx, capi, states, times)
        for key in want:
            assert got[key] == want[key], (tag, key)
            assert got[key] != first[0].get(key), (tag, key, "the reader does not see the correction")
        assert _lm(pb, k, ctx, capi) == _lm(twin, k, ctx, capi), (tag, "LM")
        print("CHAIN readers %s: %s and the LM's results and knots: the same bytes on the corrected object and on the twin updated with the corrected frames"
              % (tag, ", ".join(sorted(want))))
    finally:
        pb.close()
        twin.close()


def test_readers_on_object_a(mbavo, gpu_ctx):
    o = po.OBJECTS["A"]
    _readers_agree(mbavo, gpu_ctx, lambda: pp.make_object(gpu_ctx, "A"), pp.exposed_blur("A"), o["k"], "A", 0, min_pixels=pp.MIN_PIXELS)


def test_readers_on_the_plain_shape(mbavo, gpu_ctx):
    """With the hypothesis pick: the plain shape's knots and times as tracker states."""
    m = pp.motion(*PLAIN[:3])
    states = pp.off_knots_states(mbavo.capi, PLAIN, pair=-1)
    _readers_agree(mbavo, gpu_ctx, lambda: pp.prepared(gpu_ctx, PLAIN), pp.images()["blur"], PLAIN[0], "plain", 1, states=states,
                   times=(m["cap"], m["exp"]), min_pixels=pp.MIN_PIXELS)


def test_the_correction_ends_with_the_next_frame(mbavo, gpu_ctx):
    capi = mbavo.capi
    c = pp.images()
    new = np.ascontiguousarray(np.stack([pref.exposed(np.roll(c["sharp"][b], (-1, 2), (0, 1)), *pp.EXPOSURE[(b + 1) % pp.B]) for b in range(pp.B)]))
    # update, n_key = 0
    pb, counts = pp.prepared(gpu_ctx, PLAIN)
    twin, _ = pp.prepared(gpu_ctx, PLAIN)
    try:
        out = pp.apply(pb, counts, "lifetime update", level=0, extended=True, min_pixels=pp.MIN_PIXELS)
        assert any(r.status == 0 for r in out)
        for q in (pb, twin):
            assert np.array_equal(q.update(dv.dev(new)[0]), counts)
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(twin, counts), "lifetime update")
        pp.same_state(pp.state(pb, counts, extended=True), pp.state(twin, counts, extended=True), "lifetime update")
        assert np.array_equal(dv.read_batch(pb, counts)[0]["cur"].reshape(pp.H, pp.W), new[0])
    finally:
        pb.close()
        twin.close()
    # track_frame
    pb, counts = pp.prepared(gpu_ctx, TRACKED)
    twin, _ = pp.prepared(gpu_ctx, TRACKED)
    try:
        out = pp.apply(pb, counts, "lifetime track_frame", level=0, extended=True, min_pixels=pp.MIN_PIXELS)
        assert any(r.status == 0 for r in out)
        got = [dv.frames_of(gpu_ctx, capi, q, dict(B=pp.B), dv.dev(new)[0], (), None, None, TRACKED[0]) for q in (pb, twin)]
        assert got[0][0] == got[1][0] and got[0][2:] == got[1][2:] and np.array_equal(got[0][1], got[1][1]), "lifetime track_frame"
        dv.assert_twins(dv.read_batch(pb, counts), dv.read_batch(twin, counts), "lifetime track_frame")
        pp.same_state(pp.state(pb, counts, extended=True), pp.state(twin, counts, extended=True), "lifetime track_frame")
        print("CHAIN lifetime: after apply = 1, update (n_key = 0) and track_frame leave the bytes of a twin that was never matched")
    finally:
        pb.close()
        twin.close()


def test_apply_leaves_filter_tracker_and_hand_over_state(mbavo, gpu_ctx):
    """Two objects take filter_depths, one track_frame and a carry_save; one of them then apply = 1.  Its filter and tracker state
    keep their bytes across the call, and the hand-over state -- read once, by the report-only adopt that consumes it -- is the
    other object's."""
    capi = mbavo.capi
    c = pp.images()
    carried = [0, 2]
    made = []
    try:
        for _ in range(2):
            pb, counts = pp.prepared(gpu_ctx, TRACKED)
            made.append(pb)
            rc, fil = pb.filter_depths(level=-1, apply=True, **dc.FILTER)
            assert rc == 0 and all(f.seeded == 1 for f in fil)
            dv.frames_of(gpu_ctx, capi, pb, dict(B=pp.B), dv.dev(c["blur"])[0], (), None, None, TRACKED[0])
            rc, saved = pb.carry_save(carried, np.stack([dc.TILT, dc.rounds_poses()[1]]), radius=2, deflate=0.8)
            assert rc == 0 and sum(s.num_carried for s in saved) > 0
        pb, twin = made
        st = pp.state(pb, counts, extended=True)[2]
        assert st["filter"] is not None and st["tracker"] is not None and float(np.abs(st["filter"]["info"]).max()) > 0
        out = pp.apply(pb, counts, "state", level=0, extended=True, min_pixels=pp.MIN_PIXELS)
        assert any(r.status == 0 for r in out)
        got, want = pp.handover(pb, carried), pp.handover(twin, carried)
        assert got == want and any(v != bytes(len(v)) for v in want[0].values())
        print("CHAIN state: apply = 1 (status %s) changed no byte of the filter state, the tracker state or the hand-over state" % [r.status for r in out])
    finally:
        for pb in made:
            pb.close()


def test_apply_leaves_the_masks(mbavo, gpu_ctx):
    pb, counts = pp.make_object(gpu_ctx, "B")
    twin, _ = pp.make_object(gpu_ctx, "B")
    try:
        out = pp.apply(pb, counts, "masks", level=0, extended=True, min_pixels=pp.MIN_PIXELS)
        assert all(r.status == 0 for r in out)
        got, want = pp.masks_probe(pb, "B"), pp.masks_probe(twin, "B")
        assert got == want and got[0] == counts.tobytes()
        print("CHAIN masks: after apply = 1 a detection of every keyframe of object B selects the keypoints it selects on an untouched object")
    finally:
        pb.close()
        twin.close()


def test_report_after_a_prune(mbavo, gpu_ctx):
    import torch
    o = po.OBJECTS["A"]
    pb, counts = pp.make_object(gpu_ctx, "A")
    try:
        keeps = psup.keep_patterns(counts, psup.SEED_ALL)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(psup.SEED_ALL))
        rc, rec = pb.prune_keypoints(level=-1, apply=True, drop_mask=psup.MASK, flags=torch.from_numpy(flags).to("cuda:0"))
        now = _counts_now(pb)
        assert rc == 0 and (now < counts).all() and (now > 0).all()
        assert all(now[b, l] == int(keeps[(b, l)].sum()) for b in range(pb.B) for l in range(pb.L))
        for level in range(pb.L):
            _, worst = pp.check(mbavo, gpu_ctx, pb, now, o["k"], "A pruned", level=level, bound=pp.BOUND, extended=True, min_pixels=pp.MIN_PIXELS)
            print("CHAIN prune: object A level %d, K %s -> %s: largest relative difference %.3g (bound %.0e)" % (level, counts[:, level].tolist(), now[:, level].tolist(), worst, pp.BOUND))
    finally:
        pb.close()


def test_report_after_a_carry_to_the_next_keyframe(mbavo, gpu_ctx):
    """Object B: pair 2 saved under its own camera, its next keyframe through the update with the second frame (exposed like the
    first), the carried depths adopted; then a report-only call on every level."""
    name = "B"
    o, c, c2 = po.OBJECTS[name], po.inputs(name), dc.second_inputs(name)
    listed = dc.CARRY_PAIRS[name]
    Ts = np.stack([dc.carry_pose(gpu_ctx.lib, mbavo.capi, name, b) for b in listed])
    new_blur = np.ascontiguousarray(np.stack([pref.exposed(c["new_blur"][b], *pp.EXPOSURES[name][b]) for b in range(o["B"])]))
    pb, counts = pp.make_object(gpu_ctx, name)
    try:
        _, saved = ds.carry_save_check(pb, listed, Ts, tag=name, intr_of=lambda b: po.to_intr(o, b), **dc.SAVE)
        new = pb.update(po._t(new_blur), [2], po._t(c["new_sharp"]), po._t(c["new_depth"]))
        assert not np.array_equal(new[2], counts[2])
        po.set_motion(pb, c2["motion"])
        _, _, res = ds.carry_adopt_check(pb, listed, saved, dc.SAVE["radius"], tag=name, apply=True, **dc.ADOPT)
        assert sum(m["num_adopted"] for m in res.values()) > 0
        for level in range(pb.L):
            out, worst = pp.check(mbavo, gpu_ctx, pb, new, o["k"], "B carried", level=level, bound=pp.BOUND, extended=True, min_pixels=pp.MIN_PIXELS)
            print("CHAIN carry: object B level %d, status %s: largest relative difference %.3g (bound %.0e)" % (level, [r.status for r in out], worst, pp.BOUND))
    finally:
        pb.close()
