"""What tests/test_gpu_pairs_photo_options.py rests on, asserted without a GPU from the numpy restatements alone: the entries of
objects A - D (pairs_oracle.host_levels) under the exposed frames of tests/pairs_photo_support.py, the host library's pose entries
(pairs_refine_ref.poses) and the restated fit (tests/pairs_photo_ref.py).

Knife edges.  The six sums of the fit are aggregates: one item that the device decides the other way moves all of them, and no item
can be left out of a sum.  So the condition is zero cases, not a share: in every round 0 .. 7, no item of any (object, pair, level)
has a truncated-pixel coordinate within EDGE = 1e-9 of an integer or a tap coordinate within 1e-9 of 0, W - 1 or H - 1
(pairs_depth_support.knife: neither depends on the round), or a fit residual |e| within 1e-9 huber of huber or of sqrt(2) huber
(huber_weight switches where e e / 2 > huber huber).  The exposures and seeds were chosen so; a violation is answered by another
choice, never by a wider margin.

What makes the GPU file meaningful: every (pair, level) has status 0 at 1, 3 and 8 rounds; on some (object, level) 0 < num_full <
K; in the last round the share of Huber weights below 1 lies strictly between 0 and 1 on every object; two consecutive rounds' gains
differ by more than 1e-6 (relative) on some pair; a restatement under the neighbour's camera misses the gain by far more than the
bound (B, D); and every later-round case of pairs_photo_support.LATER is degenerate under the restatement, at the round stated."""
import numpy as np
import pytest

import pairs_depth_support as ds
import pairs_oracle as po
import pairs_photo_ref as pref
import pairs_photo_support as pp
import pairs_refine_ref as ref

NAMES = sorted(po.OBJECTS)
_DONE = {}


def _fits(mbavo, name):
    """Per (pair, level): the entry, its items, the restated fit at 8 rounds under wide limits (whose trace holds every round of
    the shorter fits: a round's input does not depend on the rounds behind it) and the fits at 1, 3 and 8 rounds under the defaults."""
    if name in _DONE:
        return _DONE[name]
    lib, capi, k = mbavo.load(), mbavo.capi, po.OBJECTS[name]["k"]
    out = {}
    for b, pair in enumerate(pp.host_levels(name)):
        for l, e in enumerate(pair):
            assert ref.on_knots(e, k)
            poses = ref.poses(lib, capi, e, k)
            s, c, ok = pref.items(e, poses)
            cap = max(e["K"], 1)  # (the sums' grid matters to no decision)
            fit = lambda s=s, c=c, ok=ok, e=e, cap=cap, **kw: pref.fit_items(s, c, ok, e["P"], cap, e["huber"], min_pixels=pp.MIN_PIXELS, **kw)
            out[(b, l)] = dict(e=e, s=s, c=c, ok=ok, full=ok.all(1), edge=ds.knife(e, poses, margin=pp.EDGE), wide=fit(rounds=8, **pp.WIDE),
                               fits={R: fit(rounds=R) for R in pp.ROUNDS}, fit=fit)
    _DONE[name] = out
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_exposures_are_as_the_gpu_file_needs_them(name):
    ex = pp.EXPOSURES[name]
    assert len(ex) == po.OBJECTS[name]["B"]
    assert any(a < 1 and b > 0 for a, b in ex) and any(a > 1 for a, b in ex) and (1.0, 0.0) in ex
    blur, raw = pp.exposed_blur(name), po.inputs(name)["blur"]
    for b, (a, off) in enumerate(ex):
        assert np.array_equal(blur[b], raw[b]) == ((a, off) == (1.0, 0.0)), (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_no_item_lies_on_a_knife_edge_in_any_round(mbavo, name):
    for (b, l), f in _fits(mbavo, name).items():
        assert not f["edge"].any(), (name, b, l, int(f["edge"].sum()))
        huber, nearest = f["e"]["huber"], np.inf
        for r, (ga, gb, _) in enumerate(f["wide"]["trace"] + [(f["wide"]["gain"], f["wide"]["offset"], None)]):
            e = np.abs(f["c"] - (ga * f["s"] + gb))[f["ok"]]
            for at in (huber, np.sqrt(2.0) * huber):
                d = float(np.abs(e - at).min()) if e.size else np.inf
                assert d > pp.EDGE * huber, (name, b, l, r, at, d)
                nearest = min(nearest, d)
        print("%s pair %d level %d: no keypoint of %d on a pixel or tap edge; the nearest |e| to a Huber edge in 9 residual sets: %.3g grey levels"
              % (name, b, l, f["e"]["K"], nearest))


@pytest.mark.parametrize("name", NAMES)
def test_every_pair_is_fitted_and_the_reweighting_is_active(mbavo, name):
    fits = _fits(mbavo, name)
    shares, moved = [], 0.0
    for (b, l), f in fits.items():
        for R, fit in f["fits"].items():
            assert fit["status"] == 0 and fit["num_pixels"] >= pp.MIN_PIXELS, (name, b, l, R, fit["status"])
            assert len(fit["trace"]) == (R or 3)
        last = f["fits"][0]
        a, off, _ = last["trace"][-1]
        w = ref.huber(f["c"] - (a * f["s"] + off), f["e"]["huber"])[0][f["full"]]
        shares.append(float((w != 1.0).mean()))
        g = [x[0] for x in pp.gains(f["wide"])]
        moved = max(moved, max(abs(g[r + 1] - g[r]) / abs(g[r]) for r in range(len(g) - 1)))
        print("%s pair %d level %d: K %d full %d, gains by round %s, weights other than 1 in the last round: %.3f"
              % (name, b, l, f["e"]["K"], last["num_full"], " ".join("%.6f" % v for v in g), shares[-1]))
    assert all(0.0 < s < 1.0 for s in shares), (name, shares)
    assert moved > 1e-6, (name, moved)


def test_the_full_rule_is_exercised(mbavo):
    partly = [(name, b, l) for name in NAMES for (b, l), f in _fits(mbavo, name).items() if 0 < f["fits"][0]["num_full"] < f["e"]["K"]]
    print("(object, pair, level) with 0 < num_full < K:", partly)
    assert partly


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_neighbours_camera_shows_in_the_gain(mbavo, name):
    lib, capi, o = mbavo.load(), mbavo.capi, po.OBJECTS[name]
    fits = _fits(mbavo, name)
    for l in range(o["L"]):
        e, other = fits[(0, l)]["e"], fits[(1, l)]["e"]
        wrong = pref.fit(lib, capi, dict(e, intr=other["intr"]), o["k"], max(e["K"], 1), min_pixels=pp.MIN_PIXELS)
        right = fits[(0, l)]["fits"][0]
        d = abs(wrong["gain"] - right["gain"]) / abs(right["gain"])
        print("%s level %d: pair 0 with pair 1's camera: gain %.9f against %.9f, %.3g apart" % (name, l, wrong["gain"], right["gain"], d))
        assert wrong["status"] == 0 and d > pp.WRONG_CAMERA, (name, l, d)


@pytest.mark.parametrize("case", range(len(pp.LATER)))
def test_the_later_round_cases_fail_where_they_say(mbavo, case):
    name, level, pair, kind, want_round = pp.LATER[case]
    fits = _fits(mbavo, name)
    f = fits[(pair, level)]
    found = pp.later_round_limit(f["wide"], kind)
    assert found is not None, (name, level, pair, kind, pp.gains(f["wide"]))
    limit, r = found
    assert r == want_round >= 1
    for R in (3, 8):
        got = f["fit"](rounds=R, **limit)
        assert got["status"] == pp.DEGENERATE and pp.failing_round(got) == r, (name, R, got["status"], len(got["trace"]))
        assert (got["gain"], got["offset"]) == (1.0, 0.0) and got["cost_after"] == got["cost_before"] == f["fits"][0 if R == 3 else R]["cost_before"]
    others = {b: pp.inside(fits[(b, level)]["wide"], limit, 8) for b in range(po.OBJECTS[name]["B"]) if b != pair}
    print("%s level %d pair %d: %s makes round %d degenerate (the rounds give %s); pairs that stay inside the limit in all 8 rounds: %s"
          % (name, level, pair, limit, r, ["%.6f" % x[2 if kind == "min_var" else 0] for x in pp.gains(f["wide"])[:4]], others))
    assert any(others.values()), (name, "no other pair stays inside the limit", others)
