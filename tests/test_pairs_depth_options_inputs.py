"""What tests/test_gpu_pairs_depth_options.py and tests/test_gpu_pairs_depth_rounds.py rest on, asserted without a GPU from the numpy
restatements alone: pairs_oracle.host_levels of objects A - D, the rounds object's point lists (tests/pairs_depth_cases.py) and the
host library's pose entries (pairs_refine_ref.poses).  No (pair, level) loses all full keypoints; the share of keypoints on a knife
edge (pairs_depth_support.knife) is at most 1 % everywhere, at the entry's depths and at the search's candidates; every stage takes
both sides of its decisions on these inputs; a refinement with the neighbour's camera differs visibly from the right one; and the
row-blocked neighbour search of pairs_smooth_ref equals the full one element for element."""
import numpy as np
import pytest

import pairs_carry_ref as cref
import pairs_depth_cases as dc
import pairs_depth_support as ds
import pairs_filter_ref as fref
import pairs_oracle as po
import pairs_refine_ref as ref
import pairs_search_ref as sref
import pairs_smooth_ref as mref

NAMES = sorted(po.OBJECTS)
ALL = NAMES + ["rounds"]
_DONE = {}


def _levels(name):
    """[pair][level] host entries, with k in every dict."""
    if name == "rounds":
        return [[e] for e in dc.rounds_entries()]
    return po.host_levels(name)


def _k(name):
    return dc.ROUNDS["k"] if name == "rounds" else po.OBJECTS[name]["k"]


def _stages(mbavo, name):
    """Per (pair, level) the restatements of refine, filter (two calls), search (absolute and relative), and the knife masks; made
    once per object."""
    if name in _DONE:
        return _DONE[name]
    lib, capi, k = mbavo.load(), mbavo.capi, _k(name)
    out = {}
    for b, pair in enumerate(_levels(name)):
        for l, e in enumerate(pair):
            cap = max(e["K"], 1)  # (the sums' grid matters to no decision)
            r = ref.refine(lib, capi, e, k, cap, **dc.REFINE)
            f1 = fref.filter(lib, capi, e, k, cap, fref.empty_state(e["K"]), True, **dc.FILTER)
            f2 = fref.filter(lib, capi, dict(e, z=f1["z_new"]), k, cap, f1["state"], False, **dc.FILTER)
            s, edge = {}, ds.knife_of(lib, capi, e, k)
            for relative, (lo, hi) in enumerate((dc.ABSOLUTE, dc.RELATIVE)):
                s[relative] = sref.search(lib, capi, e, k, cap, dc.ND, lo, hi, relative, min_ratio=dc.MIN_RATIO)
                edge = edge | ds.knife_of(lib, capi, e, k, zs=s[relative]["D"])
            out[(b, l)] = dict(e=e, refine=r, filters=(f1, f2), search=s, edge=edge)
    _DONE[name] = out
    return out


@pytest.mark.parametrize("name", ALL)
def test_every_entry_keeps_full_keypoints_and_few_lie_on_a_knife_edge(mbavo, name):
    for (b, l), s in _stages(mbavo, name).items():
        K, full, edge = s["e"]["K"], int(s["refine"]["full"].sum()), int(s["edge"].sum())
        print("%s pair %d level %d: K %d, full %d, on a knife edge %d" % (name, b, l, K, full, edge))
        assert s["refine"]["status"] == 0 and full > 0, (name, b, l)
        assert edge <= ds.MAX_SHARE * K, (name, b, l, edge, K)
    if name == "rounds":
        assert [s["e"]["K"] for s in _stages(mbavo, name).values()] == list(dc.ROUNDS["KS"])
        for xy, z in dc.rounds_lists():
            shared = len(z) - len(np.unique(xy, axis=0))
            bad = ~(np.isfinite(z) & (z > 0))
            assert 0.03 * len(z) < shared < 0.07 * len(z) and np.flatnonzero(bad).tolist() == dc.invalid_at(len(z))
            assert (xy == np.floor(xy)).all() and xy.min() >= 0 and xy[:, 0].max() < dc.ROUNDS["W"] and xy[:, 1].max() < dc.ROUNDS["H"]


def _decisions(mbavo, name):
    st = _stages(mbavo, name)
    count = lambda masks: sum(int(m.sum()) for m in masks)
    return dict(moved=count(s["refine"]["moved"] for s in st.values()), stays=count(~s["refine"]["moved"] for s in st.values()),
                accepted=count(s["search"][r]["accepted"] for s in st.values() for r in (0, 1)),
                refused=count(~s["search"][r]["accepted"] for s in st.values() for r in (0, 1)),
                fused=count(f["fused"] for s in st.values() for f in s["filters"]), gated=count(f["rejected"] for s in st.values() for f in s["filters"]))


@pytest.mark.parametrize("name", ALL)
def test_every_stage_takes_both_sides_of_its_decisions(mbavo, name):
    n = _decisions(mbavo, name)
    print("%s: %s" % (name, n))
    assert min(n["moved"], n["stays"], n["accepted"], n["refused"], n["fused"]) > 0, (name, n)


def test_the_gate_rejects_on_some_object(mbavo):
    gated = {name: _decisions(mbavo, name)["gated"] for name in ALL}
    assert max(gated.values()) > 0, gated


@pytest.mark.parametrize("name", NAMES)
def test_the_smoothing_has_all_three_classes_on_some_level(name):
    seen = []
    for pair in po.host_levels(name):
        for e in pair:
            m = mref.smooth(e["xy"], e["z"], **dc.smooth_opts(name))
            seen.append((m["num_supported"], m["num_filled"], m["num_outliers"]))
    print("%s: (supported, filled, outliers) per (pair, level): %s" % (name, seen))
    assert any(min(s) > 0 for s in seen), (name, seen)


def _carry(mbavo, name):
    """The restated save and adopt of the listed pairs of B or D, per (pair, level)."""
    o, lib, capi = po.OBJECTS[name], mbavo.load(), mbavo.capi
    old, new = po.host_levels(name), po.host_levels(name, dc.second_inputs(name))
    out = {}
    for b in dc.CARRY_PAIRS[name]:
        T = dc.carry_pose(lib, capi, name, b)
        for l in range(o["L"]):
            e0, e1 = old[b][l], new[b][l]
            s = cref.save(e0["xy"], e0["z"], cref.level_intrinsics(po.to_intr(o, b), l), e0["W"], e0["H"], T, deflate=dc.SAVE["deflate"])
            out[(b, l)] = (s, cref.adopt(e1["xy"], e1["z"], s, dc.SAVE["radius"], **dc.ADOPT))
    return out


@pytest.mark.parametrize("name", sorted(dc.CARRY_PAIRS))
def test_the_carry_carries_and_adopts_some_and_not_others(mbavo, name):
    carried = dropped = adopted = left = 0
    for (b, l), (s, m) in _carry(mbavo, name).items():
        print("%s pair %d level %d: carried %d of %d, adopted %d of %d" % (name, b, l, s["num_carried"], s["num_keypoints"], m["num_adopted"], m["num_keypoints"]))
        carried, dropped = carried + s["num_carried"], dropped + s["num_keypoints"] - s["num_carried"]
        adopted, left = adopted + m["num_adopted"], left + m["num_keypoints"] - m["num_adopted"]
    assert min(carried, dropped, adopted, left) > 0, (name, carried, dropped, adopted, left)


def test_the_rounds_carry_carries_and_adopts_some_and_not_others():
    (xy0, z0), (xy1, z1) = dc.rounds_lists(0)[1], dc.rounds_lists(1)[1]
    s = cref.save(xy0, z0, dc.rounds_intr(), dc.ROUNDS["W"], dc.ROUNDS["H"], dc.rounds_poses()[1], deflate=dc.SAVE["deflate"])
    some = slice(0, 600)
    m = cref.adopt(xy1[some], z1[some], s, dc.SAVE["radius"], **dc.ADOPT)
    assert 0 < s["num_carried"] < s["num_keypoints"] and 0 < m["num_adopted"] < m["num_keypoints"]


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_neighbours_camera_shows_in_the_refinement(mbavo, name):
    lib, capi, o = mbavo.load(), mbavo.capi, po.OBJECTS[name]
    levels = po.host_levels(name)
    for l in range(o["L"]):
        e, other = levels[0][l], levels[1][l]
        right = ref.refine(lib, capi, e, o["k"], max(e["K"], 1))
        wrong = ref.refine(lib, capi, dict(e, intr=other["intr"]), o["k"], max(e["K"], 1))
        d = ds.rel(wrong["g"], right["g"])
        print("%s level %d: pair 0 with pair 1's camera: g differs by %.3g of its largest" % (name, l, d))
        assert d > 1e-6, (name, l, d)


def test_the_blocked_neighbour_search_equals_the_full_one(monkeypatch):
    rng = np.random.default_rng(4)
    K = 700
    xy = np.stack([rng.integers(0, 64, K), rng.integers(0, 48, K)], 1).astype(np.float64)
    z = dc.surface_depths(rng, K)
    z[[3, 50, 333, K - 1]] = [np.nan, np.inf, 0.0, -2.0]
    w = mref.clean_weights(np.where(rng.uniform(size=K) < 0.05, 0.0, rng.uniform(0.2, 3.0, K)))
    I = rng.integers(0, 256, K).astype(np.uint8)
    valid = np.isfinite(z) & (z > 0)
    for radius, gate in ((2, 0), (3, 12), (16, 0)):
        full = mref.neighbours(xy, valid, w, I, radius, gate)
        for block in (1, 64, 97, 700, 1000):
            rows = np.concatenate([mref.neighbour_rows(xy, valid, w, I, radius, gate, i0, i0 + block) for i0 in range(0, K, block)])
            assert rows.shape == full.shape and np.array_equal(rows, full), (radius, gate, block)
    # `smooth` gives the same answer whatever the block
    want = mref.smooth(xy, z, weights=w, I=I, max_intensity_diff=12, **dc.SMOOTH)
    monkeypatch.setattr(mref, "BLOCK_CELLS", 97 * K)
    got = mref.smooth(xy, z, weights=w, I=I, max_intensity_diff=12, **dc.SMOOTH)
    assert all(np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True) for key in want)
