"""What tests/test_gpu_pairs_prune_options.py and tests/test_gpu_pairs_hyp_options.py rest on, asserted without a GPU from
pairs_oracle.host_levels of objects A - D alone (the numpy restatements that are byte-exact to the device), mbavo_pairs_plan (host
arithmetic) and the oracle.

The prune.  Object D has three levels whose K differ pairwise inside at least two pairs and capacities for which the third offset
of the level = -1 layout coincides with no wrong one; C's level 0 holds more than 4096 keypoints, some (pair, level) holds a K that
is no multiple of 64 and one fewer than 256; every keep pattern of the GPU file (pairs_prune_support.keep_patterns with its seeds)
leaves 0 < kept < K on every (pair, level) with more than one keypoint; min_keep = MIN_KEEP_D serves and skips levels of D, both
inside one pair; and on D the restatement of level 1 fed level 2's flag bytes gives other keep bytes on every pair.

The hypotheses (pairs_hyp_support: object_states, object_times, hypotheses), run through the oracle on the host levels with the
times a hypothesis call publishes: on every object, level and pair, for M = 3 and 16, the two best eligible scores differ by more
than 1 % (the precondition tests/test_pairs_hyp_api.py asserts for the existing cases), the flung-out hypothesis has no valid pixel
and every other one is eligible; some pair's winner is not 0; on D's level 2 the same holds on the pruned sets; and on B and D pair
0's score under pair 1's intrinsics differs from its own by far more than 100 x SCORE_REL.  The seeds, twists and scales of
pairs_hyp_support were chosen here until this held for every pair: none is left out."""
import numpy as np
import pytest

import pairs_hyp_ref as hr
import pairs_hyp_support as hs
import pairs_oracle as po
import pairs_prune_ref as pref
import pairs_prune_support as psup

NAMES = sorted(po.OBJECTS)


def _Ks(name):
    return np.array([[e["K"] for e in pair] for pair in po.host_levels(name)])


# ---------------------------------------------------------------------------------------------------------------- the prune
def test_object_d_tells_the_slots_apart(mbavo):
    o, Ks = po.OBJECTS["D"], _Ks("D")
    cap = psup.object_capacities(mbavo, "D")
    print("D: K %s, capacities %s" % (Ks.tolist(), cap))
    assert o["L"] == 3 and Ks.shape == (o["B"], 3) and len(cap) == 3
    assert sum(len(set(row.tolist())) == 3 for row in Ks) >= 2
    assert len(set(cap)) == 3 and sum(cap[:2]) != 2 * cap[1] and sum(cap[:2]) != 2 * cap[0] and sum(cap[:2]) != cap[2]
    assert (Ks <= np.array(cap)).all()


def test_the_sizes_the_kernel_takes_other_paths_at(mbavo):
    Ks = {name: _Ks(name) for name in NAMES}
    assert (Ks["C"][:, 0] > 4096).all()
    every = np.concatenate([k.ravel() for k in Ks.values()])
    assert (every % 64 != 0).any() and (every < 256).any() and (every > 256).any() and (every > 1).all()
    for name in NAMES:  # (a row of the caller's bytes holds every level's capacity)
        cap = psup.object_capacities(mbavo, name)
        assert len(cap) == po.OBJECTS[name]["L"] and (Ks[name] <= np.array(cap)).all(), (name, cap)


def _patterns(name):
    """(tag, keeps) of every pattern the GPU file uses on the object."""
    Ks, L = _Ks(name), po.OBJECTS[name]["L"]
    out = [("every level", psup.keep_patterns(Ks, psup.SEED_ALL))]
    out += [("level %d" % l, psup.keep_patterns(Ks, psup.SEED_LEVEL + l, levels=[l])) for l in range(L)]
    if name in ("B", "D"):
        out.append(("with a state", psup.keep_patterns(Ks, psup.SEED_FILTER)))
    if name == "D":
        out += [("min_keep", psup.keep_patterns(Ks, psup.SEED_MIN_KEEP)), ("wrong slot", psup.keep_patterns(Ks, psup.SEED_SLOT))]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_keep_pattern_keeps_some_and_drops_some(name):
    Ks = _Ks(name)
    for tag, keeps in _patterns(name):
        assert len(keeps) > 0
        for (b, l), keep in keeps.items():
            assert len(keep) == Ks[b, l] and (Ks[b, l] <= 1 or 0 < keep.sum() < Ks[b, l]), (name, tag, b, l, int(keep.sum()), int(Ks[b, l]))
    assert 0 <= psup.LEFT_OUT < Ks.shape[0] and len(psup.listed_pairs(Ks.shape[0])) == Ks.shape[0] - 1


def test_min_keep_splits_the_levels_of_d():
    Ks = _Ks("D")
    keeps = psup.keep_patterns(Ks, psup.SEED_MIN_KEEP)
    kept = np.array([[int(keeps[(b, l)].sum()) for l in range(Ks.shape[1])] for b in range(Ks.shape[0])])
    skipped = kept < psup.MIN_KEEP_D
    print("D: survivors %s against min_keep %d" % (kept.tolist(), psup.MIN_KEEP_D))
    assert skipped.any() and (~skipped).any() and any(0 < row.sum() < len(row) for row in skipped)
    assert (kept != psup.MIN_KEEP_D).any() and (kept < Ks).all()


def test_a_wrong_slot_shows_in_the_keep_bytes(mbavo):
    levels, Ks = po.host_levels("D"), _Ks("D")
    cap = psup.object_capacities(mbavo, "D")
    off = [sum(cap[:l]) for l in range(3)]
    keeps = psup.keep_patterns(Ks, psup.SEED_SLOT)
    flags = psup.flag_bytes(Ks.shape[0], cap, keeps, np.random.default_rng(psup.SEED_SLOT))
    assert flags.shape == (Ks.shape[0], sum(cap))
    for b in range(Ks.shape[0]):
        e = levels[b][1]
        right = pref.prune(e["K"], e["xy"], e["z"], None, flags=flags[b, off[1]:off[1] + cap[1]], apply=0, drop_mask=psup.MASK)
        assert np.array_equal(right["keep"].astype(bool), keeps[(b, 1)])
        for tag, wrong_off in (("level 2's slot", off[2]), ("the slot of equal capacities", 2 * cap[1]), ("level 0's slot", off[0])):
            wrong = pref.prune(e["K"], e["xy"], e["z"], None, flags=flags[b, wrong_off:wrong_off + cap[1]], apply=0, drop_mask=psup.MASK)
            assert not np.array_equal(wrong["keep"], right["keep"]), (b, tag)


# ---------------------------------------------------------------------------------------------------------------- the hypotheses
_SCORED = {}


def _scored(orc, mbavo, name, M, level, entries=None):
    """Per pair (scores, valids, eligible, winner) of the oracle on the host entries under the restated candidates."""
    key = (name, M, level, entries is not None)
    if key in _SCORED:
        return _SCORED[key]
    lib, capi = mbavo.load(), mbavo.capi
    levels = po.host_levels(name)
    states = hs.object_states(capi, name)
    cap, exp = hs.object_times(name)
    scales, twists, flung = hs.hypotheses(name, M)
    out = []
    for b in range(po.OBJECTS[name]["B"]):
        e = hs.host_entry(name, levels, b, level) if entries is None else entries[b]
        cs = hr.candidates(lib, capi.dp, states[b], cap[b], scales, twists)
        scores, valids, elig, _ = hr.oracle_scores(orc, e, cs)
        out.append((scores, valids, elig, hr.winner(scores, elig)[0], e))
    _SCORED[key] = out
    return out


def _good(name, M, level, scored, tag=""):
    flung = hs.hypotheses(name, M)[2]
    for b, (scores, valids, elig, w, e) in enumerate(scored):
        KP = float(e["K"]) * e["P"]
        order = sorted(s for s, ok in zip(scores, elig) if ok)
        print("%s%s M %d level %d pair %d: K %d, winner %d, best two %.5g %.5g, valid / KP %.2f .. %.2f"
              % (name, tag, M, level, b, e["K"], w, order[0], order[1], min(v for m, v in enumerate(valids) if m != flung) / KP, max(valids) / KP))
        assert valids[flung] == 0 and not elig[flung] and w != flung, (name, M, level, b)
        assert all(elig[m] for m in range(M) if m != flung), (name, M, level, b, valids, KP)
        assert order[1] - order[0] > 0.01 * order[1], (name, M, level, b, order[:2])


@pytest.mark.parametrize("name", NAMES)
def test_the_hypothesis_sets_are_good_ones(orc, mbavo, name):
    o = po.OBJECTS[name]
    assert hs.hypotheses(name, 1) == ([], [], None)
    cap, exp = hs.object_times(name)
    assert all(e["k"] <= e["N"] for pair in po.host_levels(name) for e in pair) and cap.shape == exp.shape == (o["B"],)
    states = hs.object_states(mbavo.capi, name)
    assert all(np.abs(np.array(st.velocity)).min() > 0 and st.N == o["N"] and st.prev_timestamp == cap[b] - hs.DT_FRAME for b, st in enumerate(states))
    winners = []
    for M in hs.MS[1:]:
        scales, twists, flung = hs.hypotheses(name, M)
        assert len(scales) == len(twists) == M - 1 and flung == M - 1 and twists[flung - 1] == hs.FLING
        for level in range(o["L"]):
            scored = _scored(orc, mbavo, name, M, level)
            _good(name, M, level, scored)
            winners += [s[3] for s in scored]
    assert any(w != 0 for w in winners), (name, winners)
    print("%s: winners %s" % (name, winners))


def test_the_hypothesis_set_is_good_on_the_pruned_level_of_d(orc, mbavo):
    name, level, M = "D", 2, 16
    levels, Ks = po.host_levels(name), _Ks(name)
    keeps = psup.keep_patterns(Ks, psup.SEED_ALL)
    entries = []
    for b in range(Ks.shape[0]):
        e = hs.host_entry(name, levels, b, level)
        if b in psup.listed_pairs(Ks.shape[0]):
            keep = keeps[(b, level)]
            e.update(K=int(keep.sum()), xy=np.ascontiguousarray(e["xy"][keep]), z=np.ascontiguousarray(e["z"][keep]))
        entries.append(e)
    assert [e["K"] for e in entries] != Ks[:, level].tolist()
    _good(name, M, level, _scored(orc, mbavo, name, M, level, entries), " pruned")


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_neighbours_camera_shows_in_the_score(orc, mbavo, name):
    lib, capi, o = mbavo.load(), mbavo.capi, po.OBJECTS[name]
    levels = po.host_levels(name)
    states = hs.object_states(capi, name)
    cap, exp = hs.object_times(name)
    scales, twists, flung = hs.hypotheses(name, 3)
    cs = hr.candidates(lib, capi.dp, states[0], cap[0], scales, twists)
    for level in range(o["L"]):
        e, other = hs.host_entry(name, levels, 0, level), levels[1][level]["intr"]
        right = hr.oracle_scores(orc, e, cs)[0]
        wrong = hr.oracle_scores(orc, dict(e, intr=other), cs)[0]
        for m in range(3):
            if m != flung:
                d = abs(wrong[m] - right[m]) / abs(right[m])
                print("%s level %d hypothesis %d: pair 0 under pair 1's camera: the score differs by %.3g" % (name, level, m, d))
                assert d > 1e4 * hr.SCORE_REL, (name, level, m, d)
