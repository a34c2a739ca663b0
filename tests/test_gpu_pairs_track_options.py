"""The pairs tracker -- mbavo_pairs_assess, _predict, _commit and mbavo_pairs_track_frame -- on the option-laden objects A - D of
tests/pairs_oracle.py, held to the oracle's orc_is_keyframe, to the host algebra of tests/pairs_track.py and to
pairs_oracle.oracle_lm_levels.  The tracker's own tests build one pinhole camera, grid picks, three levels of a kind, six knots and
start index 0, and the option tests compare one device run with another; there a level taken for a pair in the counts or the device
table, a wrong pair index into the cameras, a sum that goes wrong past 16 rounds of 256 lanes or a knot boundary off by one cannot
show.  Here: per-level counts that differ from every neighbouring entry (D, and every object after a prune), camera sets (B: four
pairs on two cameras, D: three on three), level-0 lists beyond 4096 keypoints (C), the last admissible segment of a k = 4 spline (A:
idx == 1 == N - k) and the smallest spline there is (B, C: k = N = 2).  What the objects, thresholds, states and times must provide
is asserted without a GPU in tests/test_pairs_track_options_inputs.py; the helpers are in tests/pairs_track_support.py.

Bounds.  avg_flow / avg_kernel: pairs_step.bound (2^-23 relative, floor 0); the pose 1e-12; counts, the verdict (every pair passes
margin_ok) and the count of points behind the camera exact.  The pose algebra of predict and commit: pairs_track.ALGEBRA_CAP = 1e-9
absolute, not the measured algebra_bound of the plain states.  The tracked frame against the four calls: the same bytes.  Its LM
against the oracle: the comparison of tests/test_gpu_pairs_oracle.py as it stands (decisions equal, costs 1e-6, knots 1e-5).  Every
figure is printed before it is asserted (-s); the largest per object on an MI355X are in profiles/r38_track_options.txt."""
import contextlib

import numpy as np
import pytest

import pairs_oracle as po
import pairs_prune_ref as pref
import pairs_prune_support as psup
import pairs_track as pt
import pairs_track_support as tsup

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)


@contextlib.contextmanager
def _fresh(ctx, name, n=1):
    made = []
    try:
        for _ in range(n):
            made.append(po.make_object(ctx, name))
        yield made[0] if n == 1 else made
    finally:
        for pb, _ in made:
            pb.close()


def _assess_against_the_oracle(orc, mbavo, ctx, pb, name, counts0, tag):
    """Check 1 on the object as it is, under its own motion: every pair against the oracle, both verdicts, twice the same bytes."""
    m, thr = tsup.motion_of(name), tsup.THRESHOLDS[name]
    po.set_motion(pb, m)
    out = pb.assess(*thr)
    verdicts = tsup.check_object_assessment(orc, mbavo, ctx, pb, name, out, m["t0"], m["cap"], m["exp"], counts0, tag)
    assert [a.is_keyframe for a in out] == verdicts and set(verdicts) == {0, 1}, (tag, verdicts)
    assert bytes(pb.assess(*thr)) == bytes(out), tag
    assert all(pb.array[e].h_start_idx[0] == po.OBJECTS[name]["start"] for e in range(pb.B * pb.L)), tag


def _predict_assess_commit(orc, mbavo, ctx, pb, twin, name, counts0, tag):
    """Check 3 on the object as it is: set_states -> predict -> assess -> commit -> get_states against the host algebra, the
    assessment after the predict against the oracle (no margin asked: the thresholds were chosen for the objects' own motion)."""
    capi, o, thr = mbavo.capi, po.OBJECTS[name], tsup.THRESHOLDS[name]
    states = tsup.object_states(capi, name)
    cap, exp = tsup.algebra_times(name)
    figures = {}
    assert pb.set_states(states) == 0 and bytes(pb.get_states()) == bytes(states)
    want, t0, gkt, gkR, after_predict = tsup.check_predict(mbavo, ctx, pb, states, cap, exp, figures, twin=twin)
    assert all(pb.array[e].h_start_idx[0] == 0 for e in range(pb.B * pb.L)), tag  # (the spline starts at cap - exp / 2)
    ass = pb.assess(*thr)
    tsup.check_object_assessment(orc, mbavo, ctx, pb, name, ass, t0, cap, exp, counts0, tag + " after the predict", need_margin=False)
    out = pb.commit(*thr)
    verdicts = tsup.check_commit(mbavo, ctx, pb, o["k"], after_predict, t0, gkt, gkR, [w[3] for w in want], ass, out, cap, figures)
    print("%s: verdicts after the predict %s" % (tag, verdicts))
    tsup.assert_under_the_cap(figures, tag)
    return verdicts


# ---- 1. the assessment against the oracle
@pytest.mark.parametrize("name", NAMES)
def test_assessment_matches_the_oracle(orc, mbavo, gpu_ctx, name):
    with _fresh(gpu_ctx, name) as (pb, counts):
        _assess_against_the_oracle(orc, mbavo, gpu_ctx, pb, name, counts[:, 0], name)


# ---- 3. predict and commit against the host algebra
@pytest.mark.parametrize("name", NAMES)
def test_predict_and_commit_match_the_host_algebra(orc, mbavo, gpu_ctx, name):
    with _fresh(gpu_ctx, name, 2) as ((pb, counts), (twin, _)):
        verdicts = _predict_assess_commit(orc, mbavo, gpu_ctx, pb, twin, name, counts[:, 0], name)
        assert set(verdicts) == {0, 1}, (name, verdicts)  # knots re-expressed and knots left alone


def test_a_sample_past_the_last_segment_is_refused(mbavo, gpu_ctx):
    """Object A's range edge: the exposure that puts pair 1's last sample on idx == 2 (idx + k > N) makes the predict return
    MBAVO_E_RANGE with knots, times and states as they were; the longest exposure that keeps it on idx == 1 passes."""
    name = "A"
    capi = mbavo.capi
    with _fresh(gpu_ctx, name) as (pb, counts):
        states = tsup.object_states(capi, name)
        assert pb.set_states(states) == 0
        cap, exp = tsup.algebra_times(name)
        held = (bytes(pb.get_states()), [a.tobytes() for a in pb.knots()], tsup.problem_times(pb))
        bad = exp.copy()
        bad[1] = tsup.EXP_PAST_THE_KNOTS_A
        assert pb.predict(cap, bad) == tsup.E_RANGE
        assert (bytes(pb.get_states()), [a.tobytes() for a in pb.knots()], tsup.problem_times(pb)) == held
        assert held[0] == bytes(states) and pb.track_stats() == ((0, 0, 0), (0, 0, 0))
        frames = (capi.PairsFrame * pb.B)()
        thr = tsup.THRESHOLDS[name]
        assert gpu_ctx.lib.mbavo_pairs_commit(pb.handle, thr[0], thr[1], thr[2], frames) == tsup.E_ARG  # no predict is pending
        assert pb.predict(cap, exp) == 0
        out = pb.commit(*tsup.THRESHOLDS[name])
        assert all(f.a.status == 0 for f in out)


# ---- 4. after a prune
@pytest.mark.parametrize("name", NAMES)
def test_assessment_and_commit_after_a_prune(orc, mbavo, gpu_ctx, name):
    with _fresh(gpu_ctx, name, 2) as ((pb, counts), (twin, _)):
        keeps = psup.keep_patterns(counts, tsup.PRUNE_SEED)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(tsup.PRUNE_SEED))
        out, res, snap, _ = pref.run_and_check(pb, None, level=-1, apply=True, flags=flags, drop_mask=psup.MASK, tag=name + " prune")
        kept0 = np.array([int(keeps[(b, 0)].sum()) for b in range(pb.B)])
        assert ((0 < kept0) & (kept0 < counts[:, 0])).all(), (name, kept0, counts[:, 0])
        assert [res[(b, 0)]["K"] for b in range(pb.B)] == kept0.tolist()
        print("%s: level-0 K before %s, after %s" % (name, counts[:, 0].tolist(), kept0.tolist()))
        for b, (xy, z) in enumerate(tsup.pruned_level0(name)):  # the lists the CPU file's conditions were asserted on
            got = tsup.keypoints0(pb, b)
            assert np.array_equal(got[0], xy) and np.array_equal(got[1], z), (name, b)
        _assess_against_the_oracle(orc, mbavo, gpu_ctx, pb, name, kept0, name + " after the prune")
        _predict_assess_commit(orc, mbavo, gpu_ctx, pb, twin, name, kept0, name + " after the prune")


# ---- 5. one tracked frame
def _second_frame_args(name):
    """(blur, key pairs, the listed pairs' sharp images, their depth maps or point lists) of the tracked frame."""
    c = tsup.second_inputs(name)
    if name == "B":
        first = po.inputs(name)
        return po._t(c["blur"]), [2], po._t(first["new_sharp"]), po._t(first["new_depth"])
    return po._t(c["blur"]), [], None, (() if po.OBJECTS[name]["points"] else None)


@pytest.mark.parametrize("name", NAMES)
def test_one_tracked_frame(orc, mbavo, gpu_ctx, name):
    """mbavo_pairs_track_frame against update -> predict -> mbavo_lm_batch_levels -> commit on a twin, byte for byte; the twin's LM
    against the oracle on the entries rebuilt after its predict, the commit behind it against the host algebra fed with the
    device's pose."""
    capi, o, thr = mbavo.capi, po.OBJECTS[name], tsup.THRESHOLDS[name]
    states = tsup.object_states(capi, name)
    cap, exp = tsup.frame_times(name, tsup.EXP_TRACKED)
    blur, keys, sharp, extra = _second_frame_args(name)
    lm = po.lm_opts(capi, o["k"])
    with _fresh(gpu_ctx, name, 2) as ((pb, counts), (twin, _)):
        assert pb.set_states(states) == 0 and twin.set_states(states) == 0
        if o["points"]:
            frames, new_counts, res, trace = pb.track_frame_points(blur, cap, exp, lm, thr, keys, sharp, extra, trace_cap=tsup.CAP)
            twin_counts = twin.update_points(blur, keys, sharp, extra)
        else:
            frames, new_counts, res, trace = pb.track_frame(blur, cap, exp, lm, thr, keys, sharp, extra, trace_cap=tsup.CAP)
            twin_counts = twin.update(blur, keys, sharp, extra)
        assert np.array_equal(new_counts, twin_counts) and (new_counts > 0).all(), name
        assert np.array_equal(new_counts, counts) == (not keys), name
        figures = {}
        want_p, t0, gkt, gkR, after_predict = tsup.check_predict(mbavo, gpu_ctx, twin, states, cap, exp, figures)
        got = {}
        tsup.check_lm(orc, mbavo, gpu_ctx, twin, name, name + " tracked frame", start=0, got_out=got)
        lkt, lkR = twin.knots()
        assert not np.array_equal(lkt, gkt)  # (the LM moved the knots)
        ass = twin.assess(*thr)
        tsup.check_object_assessment(orc, mbavo, gpu_ctx, twin, name, ass, t0, cap, exp, new_counts[:, 0], name + " tracked frame", need_margin=False)
        hframes = twin.commit(*thr)
        # the one call and the four: the same bytes
        assert bytes(frames) == bytes(hframes), name
        assert bytes(res) == bytes(got["res"]), name
        assert tsup.trace_tuples(trace, res, pb.B) == got["records"], name
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pb.knots(), twin.knots())), name
        assert bytes(pb.get_states()) == bytes(twin.get_states()), name
        assert tsup.problem_times(pb) == tsup.problem_times(twin) and [pb.array[e].K for e in range(pb.B * pb.L)] == new_counts.ravel().tolist()
        # the commit behind the LM
        verdicts = tsup.check_commit(mbavo, gpu_ctx, twin, o["k"], after_predict, t0, lkt, lkR, [w[3] for w in want_p], ass, hframes, cap, figures)
        print("%s tracked frame: verdicts %s" % (name, verdicts))
        tsup.assert_under_the_cap(figures, name + " tracked frame")
        assert pt.ALGEBRA_CAP == 1e-9
