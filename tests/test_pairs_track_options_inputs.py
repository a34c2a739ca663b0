"""What tests/test_gpu_pairs_track_options.py rests on, asserted without a GPU from pairs_oracle.host_levels of objects A - D (the
numpy restatements that are byte-exact to the device), the oracle and the C ABI's host algebra.

The thresholds of pairs_track_support split every object -- both verdicts occur -- and every pair of every object passes
pairs_step.margin_ok: none is left out.  The comparison sees the faults it is there for: a pair assessed under a neighbour's
intrinsics (B, D), level 1's list in level 0's place (D), a neighbouring entry of the counts (D: level 0's K differs from the same
pair's level 1 and 2 and from the next pair's level 0) each move the oracle's averages by more than pairs_step.bound; C's level-0
lists are longer than 16 rounds of 256 lanes; A's three sample times lie on idx == 1 == N - k, and after a predict the exposure
EXP_LAST_SEGMENT_A puts the frame's last sample and cap + exp / 2 there, EXP_PAST_THE_KNOTS_A one segment further.  The pruned
level-0 lists move the averages by more than the bound, so a stale count or list shows.  On the tracked frame -- the second inputs
under the predicted motion -- the oracle and its contracted build take the same decisions on every pair, no patch cost lies within
1e-6 of its chi bound, accepted and rejected steps both occur and the two builds end within 3e-6 of each other in every knot: the
state seeds of pairs_track_support were chosen here."""
import numpy as np
import pytest

import pairs_oracle as po
import pairs_step as ps
import pairs_track_support as tsup

NAMES = sorted(po.OBJECTS)


def _assess(orc, name, b, xy, z, m=None, intr=None):
    o, m = po.OBJECTS[name], tsup.motion_of(name) if m is None else m
    return ps.oracle_assess(orc, po.to_intr(o, b) if intr is None else intr, xy, z, o["k"], m["t0"][b], m["dt"], m["kt"][b], m["kR"][b], m["cap"][b],
                            m["exp"][b], tsup.THRESHOLDS[name])


def _differs(a, w):
    """Both averages further apart than the bound the device is held to."""
    return abs(a[1] - w[1]) > ps.bound(w[1]) and abs(a[2] - w[2]) > ps.bound(w[2])


@pytest.mark.parametrize("name", NAMES)
def test_the_thresholds_split_every_object_and_no_pair_is_near_one(orc, name):
    levels = po.host_levels(name)
    thr = tsup.THRESHOLDS[name]
    assert thr[0] < thr[1]
    verdicts = []
    for b, pair in enumerate(levels):
        v, af, ak = _assess(orc, name, b, pair[0]["xy"], pair[0]["z"])
        print("%s pair %d: K %d flow %.6g kernel %.6g verdict %d (thresholds %s)" % (name, b, pair[0]["K"], af, ak, v, thr))
        assert ps.margin_ok(af, ak, thresholds=thr), (name, b, af, ak)
        assert min(abs(af - thr[0]), abs(af - thr[1])) > 0.01 * af and abs(ak - thr[2]) > 0.01 * ak, (name, b)  # (far from a rounding)
        verdicts.append(v)
    assert set(verdicts) == {0, 1}, (name, verdicts)


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_neighbours_intrinsics_show_in_the_assessment(orc, name):
    o = po.OBJECTS[name]
    levels = po.host_levels(name)
    seen = 0
    for b in range(o["B"]):
        e = levels[b][0]
        own = _assess(orc, name, b, e["xy"], e["z"])
        for other in range(o["B"]):
            if o["cam_of"][other] == o["cam_of"][b]:
                continue
            wrong = _assess(orc, name, b, e["xy"], e["z"], intr=po.to_intr(o, other))
            print("%s pair %d under pair %d's intrinsics: flow %.6g / %.6g kernel %.6g / %.6g" % (name, b, other, wrong[1], own[1], wrong[2], own[2]))
            assert _differs(wrong, own), (name, b, other)
            seen += 1
    assert seen >= o["B"]
    assert o["cam_of"][0] == 0 and any(g != 0 for g in o["cam_of"])  # (a kernel that took camera 0 for every pair has a pair to show on)


def test_object_d_tells_level_0_from_its_neighbours(orc):
    name, o = "D", po.OBJECTS["D"]
    levels = po.host_levels(name)
    Ks = np.array([[e["K"] for e in pair] for pair in levels])
    print("D: K %s" % Ks.tolist())
    flat = Ks.ravel()
    for b in range(o["B"]):
        i = b * o["L"]
        near = [flat[i + 1], flat[i + 2]] + ([flat[i + o["L"]]] if b + 1 < o["B"] else [])
        assert all(n != flat[i] for n in near), (b, flat[i], near)
        own = _assess(orc, name, b, levels[b][0]["xy"], levels[b][0]["z"])
        wrong = _assess(orc, name, b, levels[b][1]["xy"], levels[b][1]["z"])
        print("D pair %d on level 1's list: flow %.6g / %.6g kernel %.6g / %.6g" % (b, wrong[1], own[1], wrong[2], own[2]))
        assert _differs(wrong, own), b
        # the first K1 of level 0's list alone -- level 1's count over level 0's list -- shows as well
        short = _assess(orc, name, b, levels[b][0]["xy"][:Ks[b, 1]], levels[b][0]["z"][:Ks[b, 1]])
        assert Ks[b, 1] < Ks[b, 0] and _differs(short, own), b


def test_object_c_sums_over_more_than_sixteen_rounds():
    Ks = np.array([[e["K"] for e in pair] for pair in po.host_levels("C")])
    assert (Ks[:, 0] > 4096).all() and (Ks[:, 0] % 256 != 0).all(), Ks.tolist()


def test_object_a_meets_its_last_segment():
    o, m = po.OBJECTS["A"], tsup.motion_of("A")
    assert o["N"] - o["k"] == 1 == o["start"]
    for b in range(o["B"]):
        blur, three = tsup.sample_indices(o, m["cap"][b], m["exp"][b], m["t0"][b], m["dt"])
        assert set(blur) == {1} and three == [1, 1, 1], (b, blur, three)
    # after a predict the spline starts at cap - exp / 2
    cap, exp = tsup.algebra_times("A")
    for b in range(o["B"]):
        blur, three = tsup.sample_indices(o, cap[b], exp[b], cap[b] - 0.5 * exp[b], m["dt"])
        assert blur[0] == 0 and blur[-1] == 1 and three[2] == 1 and max(blur + three) == 1, (b, blur, three)
        blur, _ = tsup.sample_indices(o, cap[b], tsup.EXP_PAST_THE_KNOTS_A, cap[b] - 0.5 * tsup.EXP_PAST_THE_KNOTS_A, m["dt"])
        assert blur[-1] == 2 and blur[-1] + o["k"] > o["N"], (b, blur)
    for name in ("B", "C"):
        assert po.OBJECTS[name]["N"] == po.OBJECTS[name]["k"] == 2


@pytest.mark.parametrize("name", NAMES)
def test_the_pruned_lists_move_the_averages(orc, name):
    levels = po.host_levels(name)
    pruned = tsup.pruned_level0(name, levels)
    thr = tsup.THRESHOLDS[name]
    for b, (xy, z) in enumerate(pruned):
        e = levels[b][0]
        assert 0 < len(z) < e["K"], (name, b, len(z), e["K"])
        full, cut = _assess(orc, name, b, e["xy"], e["z"]), _assess(orc, name, b, xy, z)
        print("%s pair %d: K %d -> %d, flow %.6g -> %.6g, kernel %.6g -> %.6g" % (name, b, e["K"], len(z), full[1], cut[1], full[2], cut[2]))
        assert _differs(cut, full), (name, b)
        assert ps.margin_ok(cut[1], cut[2], thresholds=thr), (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_the_states_predict_to_a_frame_the_tests_can_hold(orc, mbavo, name):
    """Check 3's frame: every pair's assessment after the predict has a status of 0 by the times alone, and the velocities move every
    knot of every pair but the one at rest by far more than the algebra cap, so a knot left out of the predict shows."""
    import pairs_track as pt
    lib, capi, o = mbavo.load(), mbavo.capi, po.OBJECTS[name]
    states = tsup.object_states(capi, name)
    cap, exp = tsup.algebra_times(name)
    m = tsup.predicted_motion(lib, capi, name, states, cap, exp)
    m0 = tsup.motion_of(name)
    for b in range(o["B"]):
        blur, three = tsup.sample_indices(o, cap[b], exp[b], m["t0"][b], m["dt"])
        assert min(blur + three) >= 0 and max(blur + three) + o["k"] <= o["N"], (name, b, blur, three)
        moved = np.abs(m["kt"][b] - m0["kt"][b]).max(axis=1) + np.abs(m["kR"][b] - m0["kR"][b]).max(axis=1)
        assert (moved == 0).all() if b == 1 else (moved > 1e4 * pt.ALGEBRA_CAP).all(), (name, b, moved)
    levels = po.host_levels(name)
    verdicts = [_assess(orc, name, b, levels[b][0]["xy"], levels[b][0]["z"], m=m)[0] for b in range(o["B"])]
    assert set(verdicts) == {0, 1}, (name, verdicts)  # the commit re-expresses some pairs' knots and leaves the others' alone


_RUNS = {}


def _tracked(orc, mbavo, name):
    if name not in _RUNS:
        levels = tsup.tracked_host_levels(mbavo.load(), mbavo.capi, name)
        fma = orc.fma_variant()
        runs = {tag: None if lib is None else [po.oracle_lm_levels(lib, [po.problem_of(lib, dict(e)) for e in pair]) for pair in levels]
                for tag, lib in (("oracle", orc), ("fma", fma))}
        _RUNS[name] = dict(levels=levels, **runs)
    return _RUNS[name]


@pytest.mark.parametrize("name", NAMES)
def test_the_tracked_frames_lm_cannot_flip_on_a_rounding(orc, mbavo, name):
    o = po.OBJECTS[name]
    r = _tracked(orc, mbavo, name)
    Ks = np.array([[e["K"] for e in pair] for pair in r["levels"]])
    assert (Ks > 0).all(), (name, Ks.tolist())
    for pair in r["levels"]:
        assert all(e["start"][0] == 0 and e["t0"] == e["cap"][0] - 0.5 * e["exp"][0] for e in pair)
        blur, three = tsup.sample_indices(o, pair[0]["cap"][0], pair[0]["exp"][0], pair[0]["t0"], pair[0]["dt"])
        assert set(blur) == {0} and three[0] == 0, (name, blur, three)  # every sample of the frame on the capture time's segment
    kinds = [t[2] for a in r["oracle"] for t in a["trace"]]
    print("tracked frame %s: K %s, accepted %d rejected %d invalid %d" % (name, Ks.tolist(), kinds.count(1), kinds.count(2), kinds.count(3)))
    assert kinds.count(1) > 0 and kinds.count(2) > 0, name
    if r["fma"] is None:
        pytest.skip("the host compiler or CPU has no FMA: no contracted build to compare with")
    for b, (a, f) in enumerate(zip(r["oracle"], r["fma"])):
        assert [t[:4] for t in a["trace"]] == [t[:4] for t in f["trace"]], (name, b)
        assert a["margin"] > 1e-6 and f["margin"] > 1e-6, (name, b, a["margin"], f["margin"])
        knots = max(float(np.abs(a["kt"] - f["kt"]).max()), float(np.abs(a["kR"] - f["kR"]).max()))
        print("tracked frame %s pair %d: %d records, chi margin %.2e, quality margin %.2e, the two builds' knots %.2e apart"
              % (name, b, len(a["trace"]), a["margin"], a["quality_margin"], knots))
        assert knots < 3e-6, (name, b, knots)  # (both builds end at the same place: the seeds were chosen for it)
