"""mbavo_pairs_match_brightness on the option-laden objects A - D of tests/pairs_oracle.py, held to its numpy restatement
(tests/pairs_photo_ref.py) run on entries rebuilt from the object's own device arrays (pairs_oracle.read_entry) -- the checks of
tests/test_gpu_pairs_photo.py, shared through tests/pairs_photo_support.py.  That file builds one pinhole camera, 48 x 64 and 96 x 128
images and B = 3; here the kernel runs on a packed keyframe at 75 x 101 with start = 1, N = 5 and 16-bit depth (A), on four pairs of
a radtan and a unified camera under undistort = 2 with masks (B), on the every-candidate P = 1 unified-model object (C) and on all
three cameras of D at L = 3.  The objects' frames have no brightness change, so every pair's raw blurred frame first passes through
pairs_photo_ref.exposed with its own (gain, offset) (pairs_photo_support.EXPOSURES) and comes in by mbavo_pairs_update with n_key = 0.
What these inputs must provide is asserted without a GPU in tests/test_pairs_photo_options_inputs.py.

Bounds.  status, num_keypoints, num_full and num_pixels are identical.  gain, cost_before, cost_after: |device - restatement| /
|restatement|; offset: |device - restatement| / max(|restatement|, 1 grey level); each within BOUND = 1e-9, the project's figure
for quantities behind the device's pose prologue (tests/test_gpu_fullsize.py, tests/test_gpu_pairs_depth_options.py) -- not a number
measured on this kernel.  No item is left out: the CPU file shows that none lies within 1e-9 of a discontinuity.  The correction is
held bit for bit to the restated correction under the DEVICE's (a, b), and everything else of the object -- entries, knots, filter
state, tracker state -- to the same bits (pairs_photo_support.state, extended).  Every figure is printed before it is asserted (-s);
the largest per object and level on an MI355X are in profiles/r43_photo_options.txt.

Later rounds.  A limit taken from the restatement's trace (pairs_photo_support.later_round_limit) lets a pair pass round 0 and makes
it degenerate in round 2; the launches behind it skip the pair before the ticket.  Its record, its frames under apply, the other
pairs' records and a default call on the same object directly afterwards -- against the same call on an object that has never run
the restricted call -- are bit for bit."""
import contextlib

import numpy as np
import pytest

import pairs_depth_support as ds
import pairs_oracle as po
import pairs_photo_ref as pref
import pairs_photo_support as pp

pytestmark = pytest.mark.gpu

NAMES = sorted(po.OBJECTS)
BOUND = pp.BOUND


@pytest.fixture(scope="module")
def made(mbavo, gpu_ctx):
    """name -> (pb, counts): each object made once for the report-only checks, closed at the end of the module."""
    held = {}

    def get(name):
        if name not in held:
            held[name] = pp.make_object(gpu_ctx, name)
        return held[name]
    yield get
    for pb, _ in held.values():
        pb.close()


@contextlib.contextmanager
def _second(make):
    """A further instance for the calls that write."""
    pb, counts = make()
    try:
        yield pb, counts
    finally:
        pb.close()


@pytest.mark.parametrize("name", NAMES)
def test_report_only(mbavo, gpu_ctx, made, name):
    o = po.OBJECTS[name]
    pb, counts = made(name)
    for level in range(o["L"]):
        log = []
        for rounds in pp.ROUNDS:
            out, _ = pp.check(mbavo, gpu_ctx, pb, counts, o["k"], "%s rounds %d" % (name, rounds or 3), level=level, bound=BOUND, extended=True, log=log,
                              rounds=rounds, min_pixels=pp.MIN_PIXELS)
            assert all(r.status == 0 for r in out), (name, level, rounds, [r.status for r in out])
        worst = {key: max(x[3][key] for x in log) for key in ("gain", "offset", "cost_before", "cost_after")}
        print("FIGURE report object %s level %d: largest relative difference over %d (pair, rounds): %s (bound %.0e)"
              % (name, level, len(log), "  ".join("%s %.3g" % kv for kv in worst.items()), BOUND))


@pytest.mark.parametrize("name", NAMES)
def test_apply(mbavo, gpu_ctx, name):
    o = po.OBJECTS[name]
    for level in sorted({0, o["L"] - 1}):
        with _second(lambda: pp.make_object(gpu_ctx, name)) as (pb, counts):
            out = pp.apply(pb, counts, "%s apply level %d" % (name, level), level=level, extended=True, min_pixels=pp.MIN_PIXELS)
            assert all(r.status == 0 for r in out)
            # (the pair with gain < 1 and a positive offset: the correction clamps at both ends or at neither; printed)
            cur = [np.asarray(x["cur"]) for x in pp.state(pb, counts)[0][::pb.L]]
            print("FIGURE apply  object %s level %d: bit for bit; level-0 pixels at 0 / 255 per pair: %s"
                  % (name, level, [(int((c == 0).sum()), int((c == 255).sum())) for c in cur]))


@pytest.mark.parametrize("name", ["B", "D"])
def test_a_wrong_camera_must_fail(mbavo, gpu_ctx, made, name):
    """The comparison sees the fault it is there for: pair 0's restatement with pair 1's intrinsics is far from the device's gain."""
    o, capi = po.OBJECTS[name], mbavo.capi
    pb, counts = made(name)
    cap = pb.capacities()
    for level in range(o["L"]):
        rc, out = pb.match_brightness(level=level, min_pixels=pp.MIN_PIXELS)
        assert rc == 0 and out[0].status == 0
        e, other = (po.read_entry(capi, pb.array[b * pb.L + level], o["k"]) for b in (0, 1))
        wrong = pref.fit(gpu_ctx.lib, capi, dict(e, intr=other["intr"]), o["k"], cap[level], min_pixels=pp.MIN_PIXELS)
        d = abs(out[0].gain - wrong["gain"]) / abs(wrong["gain"])
        print("%s level %d: the device's gain against pair 0's restatement under pair 1's camera: %.3g" % (name, level, d))
        assert d > pp.WRONG_CAMERA, (name, level, d)


def _later_rounds(mbavo, ctx, make, k, level, pair, limit, r, tag, inside_of, rounds=(3, 8)):
    """The later-round checks of the module docstring on two instances from `make`: pb takes the restricted calls, twin never does.
    inside_of(entries, R, the twin's unrestricted records) -> the pairs other than `pair` that stay inside the limit in every round (their records are the
    unrestricted call's)."""
    capi = mbavo.capi
    with _second(make) as (pb, counts), _second(make) as (twin, _):
        for R in rounds:
            for applied in (False, True):
                what = "%s rounds %d %s" % (tag, R, "apply" if applied else "report")
                kw = dict(rounds=R, min_pixels=pp.MIN_PIXELS, **limit)
                entries = [po.read_entry(capi, pb.array[b * pb.L + level], k) for b in range(pb.B)]
                rc, free = twin.match_brightness(level=level, rounds=R, min_pixels=pp.MIN_PIXELS)
                assert rc == 0
                if applied:
                    before = pp.state(pb, counts)[0]
                    out = pp.apply(pb, counts, what, level=level, extended=True, **kw)
                    after = pp.state(pb, counts)[0]
                    for l in range(pb.L):  # (pp.apply has asserted it for every uncorrected pair; once more for the one this is about)
                        assert np.array_equal(after[pair * pb.L + l]["cur"], before[pair * pb.L + l]["cur"]), (what, l)
                    pp.copy_frames(pb, twin)
                else:
                    out, _ = pp.check(mbavo, ctx, pb, counts, k, what, level=level, bound=BOUND, extended=True, **kw)
                bad = out[pair]
                assert (bad.status, bad.gain, bad.offset) == (pp.DEGENERATE, 1.0, 0.0) and ds.same(bad.cost_after, bad.cost_before), what
                assert (bad.num_keypoints, bad.num_full, bad.num_pixels) == (free[pair].num_keypoints, free[pair].num_full, free[pair].num_pixels), what
                assert ds.same(bad.cost_before, free[pair].cost_before) and free[pair].status == 0, what
                kept = inside_of(entries, R, free)
                assert kept, (what, "no other pair stays inside the limit")
                for b in kept:
                    assert bytes(out[b]) == bytes(free[b]), (what, b)
                # the kept scratch is clean: a default call, against the same call on the object that never ran the restricted one
                rc1, d1 = pb.match_brightness(level=level)
                rc2, d2 = twin.match_brightness(level=level)
                assert rc1 == 0 and rc2 == 0 and bytes(d1) == bytes(d2), what
                print("LATER %s: pair %d degenerate in round %d of %d under %s, cost %.17g kept; pairs %s the unrestricted call's bytes; the default call "
                      "afterwards the untouched object's bytes (status %s)" % (what, pair, r, R, limit, bad.cost_before, kept, [x.status for x in d1]))


@pytest.mark.parametrize("case", range(len(pp.LATER)))
def test_degenerate_in_a_later_round(mbavo, gpu_ctx, case):
    name, level, pair, kind, want_round = pp.LATER[case]
    o, capi, lib = po.OBJECTS[name], mbavo.capi, gpu_ctx.lib
    make = lambda: pp.make_object(gpu_ctx, name)
    with _second(make) as (pb, counts):  # the limit: from the restatement on the object's own device arrays
        cap = pb.capacities()
        e = po.read_entry(capi, pb.array[pair * pb.L + level], o["k"])
        wide = pref.fit(lib, capi, e, o["k"], cap[level], rounds=8, min_pixels=pp.MIN_PIXELS, **pp.WIDE)
    found = pp.later_round_limit(wide, kind)
    assert found is not None and found[1] == want_round, (name, found)
    limit, r = found

    def inside_of(entries, R, free):
        fits = {b: pref.fit(lib, capi, entries[b], o["k"], cap[level], rounds=8, min_pixels=pp.MIN_PIXELS, **pp.WIDE) for b in range(o["B"]) if b != pair}
        return [b for b, f in fits.items() if pp.inside(f, limit, R)]
    _later_rounds(mbavo, gpu_ctx, make, o["k"], level, pair, limit, r, "%s level %d %s" % (name, level, kind), inside_of)


def test_degenerate_in_a_later_round_among_shared_tiles(mbavo, gpu_ctx):
    """The every-candidate 96 x 128 shape of tests/test_gpu_pairs_photo.py (P = 8, G = 64 workgroups per pair, every workgroup more
    than one tile): in ONE launch pair 2 becomes degenerate in a later round, pair 1 is off its knots (mbavo_pairs_set_states) and
    pair 0 is fitted -- three ticket hand-overs side by side.  Pair 2 (taken as it is, its fitted gain falling from 0.92 round by
    round) gets a gain_min from its own trace; pair 0's gain (above 1 before its correction, about 1 after it) stays far above it,
    which is asserted on the device's own unrestricted records."""
    case = (2, 2, 0, 3, None, 0)
    k, capi, lib = case[0], mbavo.capi, gpu_ctx.lib

    def make():
        pb, counts = pp.prepared(gpu_ctx, case, dense=True, h=96, w=128, levels=2, thr=0.5)
        assert counts[:, 0].min() > 64 * 128 and pb.set_states(pp.off_knots_states(capi, case, pair=1)) == 0
        return pb, counts
    with _second(make) as (pb, counts):
        cap = pb.capacities()
        wide = pref.fit(lib, capi, po.read_entry(capi, pb.array[2 * pb.L], k), k, cap[0], rounds=4, min_pixels=pp.MIN_PIXELS, **pp.WIDE)
    found = pp.later_round_limit(wide, "gain_min")
    assert found is not None, pp.gains(wide)
    limit, r = found
    seen = []

    def inside_of(entries, R, free):
        seen.append((free[1].status, free[0].gain))
        assert free[1].status == pp.E_RANGE and free[0].status == 0 and free[0].gain > limit["gain_min"] + 0.05, (free[0].status, free[0].gain, limit)
        return [0]
    _later_rounds(mbavo, gpu_ctx, make, k, 0, 2, limit, r, "shared tiles gain_min", inside_of)
    print("shared tiles: pair 1's status and pair 0's gain in the unrestricted calls:", seen)
