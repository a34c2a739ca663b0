"""mbavo_pairs_predict_hypotheses on the option-laden objects A - D of tests/pairs_oracle.py.  The call builds B x M candidate
entries by copying the pair's entry of the level, scores them with that level's P and the device's count of that (pair, level); its
own tests run it on one pinhole camera with float gradients and P = 8 (tests/test_gpu_pairs_hyp.py).  Here every candidate must carry
its pair's own intrinsics (camera sets B and D), a half (B) or packed (A, D) keyframe, P = 1 with B x M entries of more than 5000
keypoints each (C), L = 3 with level = 2 (D), clearance-filtered lists (B, D), and the count a prune left behind (D).

With tracker states on the object's own motion (tests/pairs_hyp_support.py: object_states, a velocity that is not zero), M in
{1, 3, 16} and every level: M = 1 is mbavo_pairs_predict bit for bit; M > 1 is held by pairs_hyp_support.check_scores to the ORACLE on
the entry rebuilt from the object's device arrays (pairs_oracle.read_entry) with the restated candidates, and to the restated
selection rule.  The preconditions -- best and second-best eligible scores more than 1 % apart on every pair, the flung-out
hypothesis without a pixel, every other one eligible, a winner that is not 0, the neighbour's camera visible in the score -- are
asserted with the oracle on the CPU by tests/test_pairs_prune_hyp_options_inputs.py.

Bounds: valid counts exact; scores pairs_hyp_ref.SCORE_REL = 1e-9 relative; the winner's knots within
pairs_track.algebra_bound("predict_knots_*") of the host algebra's candidate; everything else identical.  The largest score figure
per object on an MI355X is in profiles/r37_prune_hyp_options.txt (printed by every test, -s)."""
import ctypes as C

import numpy as np
import pytest

import pairs_hyp_ref as hr
import pairs_hyp_support as hs
import pairs_oracle as po
import pairs_prune_ref as pref
import pairs_prune_support as psup
import pairs_track as pt

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)
CASES = [(name, M, level) for name in NAMES for M in hs.MS for level in range(po.OBJECTS[name]["L"])]


def _with_states(mbavo, ctx, name):
    pb, counts = po.make_object(ctx, name)
    states = hs.object_states(mbavo.capi, name)
    cap, exp = hs.object_times(name)
    return dict(pb=pb, counts=counts, states=states, cap=cap, exp=exp)


@pytest.fixture(scope="module")
def made(mbavo, gpu_ctx):
    """name -> dict(pb, twin, counts, states, cap, exp): two instances of each object, made on first use, closed at the end."""
    held = {}

    def get(name):
        if name not in held:
            h = _with_states(mbavo, gpu_ctx, name)
            h["twin"] = po.make_object(gpu_ctx, name)[0]
            held[name] = h
        return held[name]
    yield get
    for h in held.values():
        h["pb"].close()
        h["twin"].close()


def _problem_times(pb):
    return [(pb.array[e].t0, pb.array[e].dt, pb.array[e].h_start_idx[0]) for e in range(pb.B * pb.L)]


def _snapshot(pb):
    kt, kR = pb.knots()
    return kt.tobytes() + kR.tobytes(), bytes(pb.get_states()), _problem_times(pb)


def _device_counts(pb, level):
    """The device's counts of a level, as a count-only prune reports them."""
    return pref.device_counts(pb)[:, level].tolist()


def _check_winners(h, rec, oracle, cands, M, flung, tag):
    """Every pair: the oracle's winner, the flung-out hypothesis without a pixel and not counted, the winner's knots."""
    pb = h["pb"]
    kt, kR = pb.knots()
    for b in range(pb.B):
        scores, valids, elig, _ = oracle[b]
        w = hr.winner(scores, elig)[0]
        assert rec[b].winner == w and rec[b].status == 0, (tag, b, rec[b].winner, w)
        assert rec[b].valid[flung] == 0 and rec[b].winner != flung and rec[b].num_eligible == M - 1, (tag, b)
        dt_ = float(np.abs(kt[b].ravel() - cands[b][w][0]).max())
        dR_ = float(np.abs(kR[b].ravel() - cands[b][w][1]).max())
        assert dt_ <= pt.algebra_bound("predict_knots_t") and dR_ <= pt.algebra_bound("predict_knots_R"), (tag, b, dt_, dR_)


@pytest.mark.parametrize("name,M,level", CASES)
def test_hypotheses_on_an_option_laden_object(orc, mbavo, gpu_ctx, made, name, M, level):
    h = made(name)
    pb, twin, states, cap, exp = h["pb"], h["twin"], h["states"], h["cap"], h["exp"]
    scales, twists, flung = hs.hypotheses(name, M)
    assert pb.set_states(states) == 0
    tag = "%s M %d level %d" % (name, M, level)
    if M == 1:
        assert twin.set_states(states) == 0
        rc, rec = pb.predict_hypotheses(cap, exp, [], [], level=level)
        assert rc == 0 and twin.predict(cap, exp) == 0
        assert all(r.winner == 0 and r.status == 0 and r.num_eligible == 1 and r.num_keypoints == h["counts"][b, level] for b, r in enumerate(rec)), tag
        a, t = _snapshot(pb), _snapshot(twin)
        assert a[0] == t[0] and a[1] == t[1] and a[2] == t[2], tag
        assert a[0] != po.inputs(name)["motion"]["kt"].tobytes() + po.inputs(name)["motion"]["kR"].tobytes()  # (something moved)
        return
    rec, oracle, cands = hs.check_scores(orc, mbavo, gpu_ctx, pb, states, cap, exp, dict(scales=scales, twists=twists, level=level), tag)
    assert [r.num_keypoints for r in rec] == h["counts"][:, level].tolist() == _device_counts(pb, level), tag
    _check_winners(h, rec, oracle, cands, M, flung, tag)
    for b in range(pb.B):  # every candidate entry carried the pair's own camera and the level's own P
        q = pb.array[b * pb.L + level]
        assert list(q.intrinsics) == [v / float(1 << level) for v in po.to_intr(po.OBJECTS[name], b)] and q.P == po.OBJECTS[name]["P"], (tag, b)


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_wrong_camera_must_fail(orc, mbavo, gpu_ctx, made, name):
    """The comparison sees the fault it is there for: pair 0's oracle score under pair 1's intrinsics is far from the device's."""
    capi, h = mbavo.capi, made(name)
    pb, states, cap, exp = h["pb"], h["states"], h["cap"], h["exp"]
    scales, twists, flung = hs.hypotheses(name, 3)
    for level in range(pb.L):
        assert pb.set_states(states) == 0
        rc, rec = pb.predict_hypotheses(cap, exp, scales, twists, level=level)
        assert rc == 0
        e = po.read_entry(capi, pb.array[level], pb.k)
        other = np.array(list(pb.array[pb.L + level].intrinsics))
        assert not np.array_equal(other, e["intr"])
        cs = hr.candidates(gpu_ctx.lib, capi.dp, states[0], cap[0], scales, twists)
        right = hr.oracle_scores(orc, e, cs)[0]
        wrong = hr.oracle_scores(orc, dict(e, intr=other), cs)[0]
        for m in range(3):
            if m == flung:
                continue
            d_right = abs(rec[0].score[m] - right[m]) / abs(right[m])
            d_wrong = abs(rec[0].score[m] - wrong[m]) / abs(wrong[m])
            print("%s level %d hypothesis %d: the device's score against pair 0's oracle %.3g, under pair 1's camera %.3g" % (name, level, m, d_right, d_wrong))
            assert d_right <= hr.SCORE_REL and d_wrong > 100 * hr.SCORE_REL, (name, level, m, d_right, d_wrong)


def test_hypotheses_after_a_prune(orc, mbavo, gpu_ctx):
    """D, level 2: the candidates are scored on the keypoints and with the count the prune left."""
    name, level, M = "D", 2, 16
    h = _with_states(mbavo, gpu_ctx, name)
    pb, counts = h["pb"], h["counts"]
    try:
        listed = psup.listed_pairs(pb.B)
        keeps = psup.keep_patterns(counts, psup.SEED_ALL)
        flags = psup.flags_of(pb, keeps, np.random.default_rng(psup.SEED_ALL))
        pref.run_and_check(pb, listed, level=-1, apply=True, flags=flags, drop_mask=psup.MASK, tag="D prune before the hypotheses")
        pruned = [int(keeps[(b, level)].sum()) if b in listed else int(counts[b, level]) for b in range(pb.B)]
        assert all(0 < pruned[b] < counts[b, level] for b in listed)
        assert pb.set_states(h["states"]) == 0
        scales, twists, flung = hs.hypotheses(name, M)
        rec, oracle, cands = hs.check_scores(orc, mbavo, gpu_ctx, pb, h["states"], h["cap"], h["exp"], dict(scales=scales, twists=twists, level=level),
                                             "D level 2 after a prune")
        assert [r.num_keypoints for r in rec] == pruned == [pb.array[b * pb.L + level].K for b in range(pb.B)]
        _check_winners(h, rec, oracle, cands, M, flung, "D level 2 after a prune")
    finally:
        pb.close()


@pytest.mark.parametrize("name", NAMES)
def test_stats(mbavo, gpu_ctx, made, name):
    h = made(name)
    pb, states, cap, exp = h["pb"], h["states"], h["cap"], h["exp"]
    scales, twists, _ = hs.hypotheses(name, 3)
    level = pb.L - 1
    assert pb.set_states(states) == 0
    rc, rec = pb.predict_hypotheses(cap, exp, scales, twists, level=level)
    assert rc == 0
    first = (bytes(rec), _snapshot(pb))
    launches = hs.launches_of_last_evaluation(gpu_ctx)
    assert pb.hyp_stats() == (2 + launches, 1, pb.B * C.sizeof(mbavo.capi.PairsHyp)), (name, pb.hyp_stats(), launches)
    assert pb.set_states(states) == 0
    rc, none = pb.predict_hypotheses(cap, exp, scales, twists, level=level, want_records=False)  # h_out = NULL: nothing is waited for
    assert rc == 0 and none is None
    assert pb.hyp_stats() == (2 + hs.launches_of_last_evaluation(gpu_ctx), 0, 0), (name, pb.hyp_stats())
    assert _snapshot(pb) == first[1]
