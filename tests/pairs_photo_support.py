"""What the GPU tests of mbavo_pairs_match_brightness share beside the restatement (tests/pairs_photo_ref.py) (helper, no test in
it): the plain B = 3 shape of tests/test_gpu_pairs_photo.py and its checks of one report-only and one applying call; the read-back
of everything of an object that a call could touch; and, for the option-laden objects A - D of tests/pairs_oracle.py, the exposures,
the exposed frames, the options and the limits of tests/test_gpu_pairs_photo_options.py, which need no device, so that
tests/test_pairs_photo_options_inputs.py can assert on the CPU what the GPU file rests on.

`state(pb, counts, extended=True)` reads back, beside the entries and the knots, the depth filter's state
(pairs_depth_support.filter_state; None before the first filter_depths) and the tracker's per-pair state (mbavo_pairs_get_states;
None before the first set_states).  The hand-over state and the masks have no pointer in the ABI; each is read through the one call
that consumes it, once, as the last thing a test does with an object, and compared with the same read on a twin that took the same
calls but the one under test: `handover` is a report-only mbavo_pairs_carry_adopt of the listed pairs (every array and record; the
adopt disarms the pairs' carried sets), `masks_probe` detects every pair's keyframe anew from the object's own inputs (the masks
act through the clearance that selects keypoints) and returns the lists.

Later-round degeneracy (`later_round_limit`).  From the restatement's trace of a run under wide limits: the gains g_0, g_1, .. the
rounds produce, and the weighted variances det / n^2 they see.  A limit halfway between g_r and the extreme of the rounds before it
lets rounds 0 .. r-1 pass and fails round r; the two sides are asked to be 1e-6 (relative) apart, a thousand times the 1e-9 the
device's doubles may differ from the restatement's by, so that both take the same decision."""
import numpy as np

import pairs_depth_support as ds
import pairs_device as dv
import pairs_oracle as po
import pairs_photo_ref as pref
import pairs_refine_ref as ref
from mba_vo_amd import synth

E_ARG, E_RANGE, DEGENERATE = -1, -2, 1
B, L, H, W, CELL, THR = 3, 3, 48, 64, 8, 4.0
EXPOSURE = [(1.3, -20.0), (0.7, 15.0), (1.0, 0.0)]
_IMAGES = {}


# ---------------------------------------------------------------------------------------------------------------- the plain shape
def images(h=H, w=W):
    if (h, w) not in _IMAGES:
        rng = np.random.default_rng(42)
        octaves = (16, 8, 4) if h == H else (8, 4)
        sharp = np.stack([synth.texture_image(h, w, seed=60 + 3 * b, octaves=octaves) for b in range(B)])
        blur = np.stack([pref.exposed(np.clip(np.roll(sharp[b], (1, -1), (0, 1)).astype(np.int32) + rng.integers(-4, 5, (h, w)), 0, 255), *EXPOSURE[b])
                         for b in range(B)])
        depth = rng.uniform(1.0, 3.0, (B, h, w)).astype(np.float32)
        _IMAGES[(h, w)] = dict(sharp=np.ascontiguousarray(sharp), blur=np.ascontiguousarray(blur), depth=depth)
    return _IMAGES[(h, w)]


def motion(k, N, start):
    rng = np.random.default_rng(11)
    kt, kR = np.zeros((B, N, 3)), np.zeros((B, N, 4))
    for b in range(B):
        kt[b], kR[b] = synth.trajectory("harness", N, 0.004 * (b + 1), 0.01 * (b + 1))
        kt[b] += rng.normal(0, 0.02, 3)
    cap = (start + 0.4 + 0.05 * np.arange(B)) * 0.5
    return dict(cap=cap, exp=np.full(B, 0.04), t0=np.zeros(B), dt=0.5, kt=kt, kR=kR)


def prepared(ctx, case, sel=slice(None), dense=False, h=H, w=W, levels=L, depth=None, sharp=None, points=None, thr=THR):
    from mba_vo_amd import workloads
    k, N, start, S, pattern, fmt = case
    c, m = images(h, w), motion(k, N, start)
    n = len(range(B)[sel])
    pb = workloads.PairBatch(ctx, n, L=levels, H=h, W=w, S=S, k=k, N=N, cell=0 if dense else CELL, thresh=thr, border=1, every_candidate=dense,
                             pattern=pattern, keyframe_format=fmt)
    d = c["depth"] if depth is None else depth
    s = c["sharp"] if sharp is None else sharp
    sharp_t, blur_t = dv.dev(np.ascontiguousarray(s[sel]), np.ascontiguousarray(c["blur"][sel]))
    if points is None:
        counts = pb.prepare(sharp_t, dv.dev(np.ascontiguousarray(d[sel]))[0], blur_t)
    else:
        counts = pb.prepare_points(sharp_t, blur_t, points)
    assert pb.set_motion(m["cap"][sel], m["exp"][sel], m["t0"][sel], m["dt"], m["kt"][sel], m["kR"][sel]) == 0
    return pb, counts


def off_knots_states(capi, case, pair=1):
    """The plain shape's knots and times as tracker states, `pair`'s knots starting long after its frame (MBAVO_E_RANGE)."""
    m = motion(case[0], case[1], case[2])
    states = (capi.VoState * B)()
    for b, st in enumerate(states):
        st.t0, st.dt, st.N, st.is_first = (100.0 if b == pair else float(m["t0"][b])), m["dt"], case[1], 0
        st.knots_t[:3 * case[1]] = list(m["kt"][b].ravel())
        st.knots_R[:4 * case[1]] = list(m["kR"][b].ravel())
        st.T_keyframe[6] = st.T_prev_b2w[6] = 1.0
    return states


# ---------------------------------------------------------------------------------------------------------------- what an object holds
def handover(pb, carried):
    """The hand-over state of the listed pairs as a report-only adopt sees it: the four arrays and the records, as bytes.  Once
    per save: the adopt disarms the pairs' carried sets."""
    t = ds.carry_arrays(pb)
    rc, out = pb.carry_adopt(list(carried), apply=False, **t)
    assert rc == 0, rc
    return {key: v.cpu().numpy().tobytes() for key, v in t.items()}, bytes(out)


def state(pb, counts, extended=False):
    """Every byte of the object a call could touch: per entry (keyframe, current frame, gradients, keypoints, depths), then the knots;
    extended: then a dict of the filter's state and the tracker's per-pair state (None where the object has none yet)."""
    out = (dv.read_batch(pb, counts), pb.knots())
    if not extended:
        return out
    extra = dict(filter=None, tracker=None)
    try:
        extra["filter"] = ds.filter_state(pb)[0]
    except RuntimeError:  # (before the first filter_depths)
        pass
    try:
        extra["tracker"] = bytes(pb.get_states())
    except RuntimeError:  # (before the first set_states)
        pass
    return out + (extra,)


def same_state(a, b, tag, but_cur=()):
    """Two read-backs hold the same bits; but_cur: the pairs whose current frames may differ."""
    n_lv = len(a[0]) // len(a[1][0])
    for e, (g, w) in enumerate(zip(a[0], b[0])):
        for key in ("ref", "cur", "grad", "xy", "z"):
            if key == "cur" and e // n_lv in but_cur:
                continue
            assert dv.same_bits(g[key], w[key]), (tag, e, key)
    assert dv.same_bits(a[1][0], b[1][0]) and dv.same_bits(a[1][1], b[1][1]), (tag, "knots")
    assert len(a) == len(b), tag
    if len(a) > 2:
        x, y = a[2], b[2]
        assert (x["filter"] is None) == (y["filter"] is None), (tag, "filter")
        if x["filter"] is not None:
            for key in ("mu", "info", "n_obs", "n_rej"):
                assert dv.same_bits(x["filter"][key], y["filter"][key]), (tag, "filter", key)
        assert x["tracker"] == y["tracker"], (tag, "tracker")


def masks_probe(pb, name):
    """What the masks and the clearance select: every pair's keyframe detected anew from the object's own inputs (counts and lists
    as bytes).  Rewrites the keyframes: the last thing done with an object."""
    c = po.inputs(name)
    counts = pb.update(None, list(range(pb.B)), po._t(c["sharp"]), po._t(c["depth"]))
    got = dv.read_batch(pb, counts)
    return counts.tobytes(), b"".join(g["xy"].tobytes() + g["z"].tobytes() for g in got)


def rels(r, want):
    out = {key: abs(getattr(r, key) - want[key]) / abs(want[key]) if want[key] != 0 else abs(getattr(r, key)) for key in ("gain", "cost_before", "cost_after")}
    out["offset"] = abs(r.offset - want["offset"]) / max(abs(want["offset"]), 1.0)
    return out


def check(mbavo, ctx, pb, counts, k, tag, level=0, bound=0.0, extended=False, log=None, **kw):
    """One apply = 0 call against the restatement: integers exact, doubles within `bound`, nothing of the object changed, the
    launch count.  Returns (records, largest relative difference).  log: a list that takes (tag, pair, level, figures, restatement)."""
    capi = mbavo.capi
    cap = pb.capacities()
    entries = [po.read_entry(capi, pb.array[b * pb.L + level], k) for b in range(pb.B)]
    before = state(pb, counts, extended)
    rc, out = pb.match_brightness(level=level, **kw)
    assert rc == 0, rc
    R = kw.get("rounds", 0) or 3
    assert pb.photo_stats() == (R + 1, 1, pb.B * 48), (tag, pb.photo_stats())
    same_state(before, state(pb, counts, extended), tag)
    worst = 0.0
    for b, e in enumerate(entries):
        want = pref.fit(ctx.lib, capi, e, k, cap[level], **kw)
        r = out[b]
        got = (r.status, r.num_keypoints, r.num_full, r.num_pixels)
        assert got == (want["status"], want["num_keypoints"], want["num_full"], want["num_pixels"]), (tag, b, got, want)
        assert r.num_keypoints == counts[b, level]
        if want["status"] == E_RANGE:
            assert all(np.isnan(v) for v in (r.gain, r.offset, r.cost_before, r.cost_after)), (tag, b)
            continue
        if want["status"] == DEGENERATE:
            assert (r.gain, r.offset) == (1.0, 0.0) and ds.same(r.cost_after, r.cost_before), (tag, b)
        figures = rels(r, want)
        print("%s pair %d level %d K %d full %d status %d gain %.6f offset %+.4f cost %.6g -> %.6g: %s"
              % (tag, b, level, r.num_keypoints, r.num_full, r.status, r.gain, r.offset, r.cost_before, r.cost_after, "  ".join("%s %.3g" % kv for kv in figures.items())))
        assert all(v <= bound for v in figures.values()), (tag, b, figures, bound)
        worst = max([worst] + list(figures.values()))
        if log is not None:
            log.append((tag, b, level, figures, want))
    return out, worst


def apply(pb, counts, tag, level=0, extended=False, **kw):
    """One apply = 1 call: every level of every pair's current frame is the restated correction of the bytes before the call with
    the device's reported (a, b) -- an uncorrected pair's are those bytes -- and nothing else has changed.  Returns the records."""
    before = state(pb, counts, extended)
    rc, out = pb.match_brightness(level=level, apply=True, **kw)
    assert rc == 0, rc
    R = kw.get("rounds", 0) or 3
    assert pb.photo_stats() == (R + 1 + 1 + (pb.L - 1 + 2) // 3, 1, pb.B * 48), (tag, pb.photo_stats())
    after = state(pb, counts, extended)
    same_state(before, after, tag, but_cur=range(pb.B))
    for b in range(pb.B):
        r = out[b]
        h, w = pb.array[b * pb.L].H, pb.array[b * pb.L].W
        cur0 = before[0][b * pb.L]["cur"].reshape(h, w)
        pyr = pref.corrected_pyramid(cur0, r.gain, r.offset, pb.L) if r.status == 0 else [before[0][b * pb.L + l]["cur"] for l in range(pb.L)]
        for l in range(pb.L):
            assert np.array_equal(after[0][b * pb.L + l]["cur"], pyr[l].ravel()), (tag, b, l, r.status)
        changed = int((after[0][b * pb.L]["cur"] != before[0][b * pb.L]["cur"]).sum())
        print("%s pair %d: status %d gain %.6f offset %+.4f, %d level-0 pixels changed" % (tag, b, r.status, r.gain, r.offset, changed))
    return out


def copy_frames(src, dst):
    """dst's current-frame pyramid takes src's bytes (two objects of one shape): dst then is src as a freshly made object that has
    never been matched."""
    for e in range(src.B * src.L):
        q, p = src.array[e], dst.array[e]
        assert (q.H, q.W) == (p.H, p.W)
        cur = dv.peek(int(dv.peek(q.d_cur_imgs, 1, np.uint64)[0]), q.H * q.W, np.uint8)
        dv.poke(int(dv.peek(p.d_cur_imgs, 1, np.uint64)[0]), cur)


# ---------------------------------------------------------------------------------------------------------------- objects A - D
BOUND = 1e-9       # gain, offset, cost_before, cost_after behind the device's pose prologue (tests/test_gpu_fullsize.py)
EDGE = 1e-9        # pixels / grey levels over huber: no item may lie this near a discontinuity
MIN_PIXELS = 8     # no (pair, level) of A - D is degenerate for lack of pixels
ROUNDS = (1, 0, 8)  # (0: the default, 3)
WIDE = dict(gain_min=1e-3, gain_max=1e3, min_var=1e-9)
# per object and pair (gain, offset): one pair with gain < 1 and a positive offset (the correction then clamps at both ends), one
# with gain > 1, one as taken
EXPOSURES = dict(A=[(0.7, 15.0), (1.3, -20.0), (1.0, 0.0)], B=[(1.25, -12.0), (0.7, 15.0), (1.0, 0.0), (0.85, 9.0)],
                 C=[(1.0, 0.0), (0.75, 20.0), (1.2, -15.0)], D=[(1.3, -20.0), (1.0, 0.0), (0.7, 15.0)])
_EXPOSED = {}


def exposed_blur(name):
    """The object's own raw blurred frames as cameras with EXPOSURES[name] would have taken them (made once)."""
    if name not in _EXPOSED:
        c = po.inputs(name)
        _EXPOSED[name] = np.ascontiguousarray(np.stack([pref.exposed(c["blur"][b], *EXPOSURES[name][b]) for b in range(len(c["blur"]))]))
    return _EXPOSED[name]


def host_levels(name):
    """pairs_oracle.host_levels of the object under the exposed frames."""
    return po.host_levels(name, dict(po.inputs(name), blur=exposed_blur(name)))


def make_object(ctx, name):
    """pairs_oracle.make_object, then the exposed frames through mbavo_pairs_update with n_key = 0 (under undistort != 0 through
    the object's own remap)."""
    pb, counts = po.make_object(ctx, name)
    try:
        again = pb.update(po._t(exposed_blur(name)))
        assert np.array_equal(again, counts)
    except Exception:
        pb.close()
        raise
    return pb, counts


def round_items(lib, capi, e, k):
    """(s, c, ok, full) of an entry under the restatement."""
    s, c, ok = pref.items(e, ref.poses(lib, capi, e, k))
    return s, c, ok, (ok.all(1) if len(ok) else np.zeros(0, bool))


def gains(fit):
    """What the rounds of a restated fit produce: [(gain_r, offset_r, det_r / n_r^2)] from its trace."""
    out = []
    for _, _, v in fit["trace"]:
        det, a, b = pref.solve(*v[:5])
        out.append((a, b, det / (v[0] * v[0])))
    return out


def later_round_limit(fit, kind, last=2, apart=1e-6):
    """(option dict, round) that makes the pair of a wide-limits restated fit degenerate in round r, 1 <= r <= last, and in no
    earlier one; kind: "gain_max", "gain_min" or "min_var".  None where the trace offers none with both sides `apart` (relative)
    from the limit."""
    g = gains(fit)
    col = 2 if kind == "min_var" else 0
    v = [x[col] for x in g]
    for r in range(min(last, len(v) - 1), 0, -1):
        if kind == "gain_max":
            side, ok = max(v[:r]), v[r] > max(v[:r])
        else:  # (a gain below gain_min, a variance not above min_var)
            side, ok = min(v[:r]), v[r] < min(v[:r])
        mid = 0.5 * (side + v[r])
        if ok and abs(v[r] - side) > 2 * apart * abs(mid):
            return {kind: mid}, r
    return None


def failing_round(fit):
    """The round at which a restated fit became degenerate: the length of its trace - 1."""
    assert fit["status"] == DEGENERATE
    return len(fit["trace"]) - 1


def inside(fit, limit, rounds, apart=1e-6):
    """Whether every one of the first `rounds` rounds of a wide-limits restated fit stays on the passing side of `limit` (one of
    gain_min, gain_max, min_var beside the defaults of the others) by more than `apart` (relative)."""
    lo, hi, var = limit.get("gain_min", pref.DEFAULTS["gain_min"]), limit.get("gain_max", pref.DEFAULTS["gain_max"]), limit.get("min_var", pref.DEFAULTS["min_var"])
    return fit["status"] == 0 and all(a > lo * (1 + apart) and a < hi * (1 - apart) and v > var * (1 + apart) and np.isfinite(b) for a, b, v in gains(fit)[:rounds])


# (object, level, pair, the limit that is set, the round that then fails): chosen on the CPU from the restatement's traces
# (tests/test_pairs_photo_options_inputs.py asserts each)
LATER = [("A", 0, 0, "gain_min", 2), ("B", 0, 0, "gain_max", 2), ("C", 0, 2, "gain_min", 2), ("D", 1, 0, "min_var", 2), ("D", 0, 0, "gain_max", 2)]
WRONG_CAMERA = 1e-6  # a restatement under the neighbour's camera misses the gain by more than this (relative): a thousand bounds
