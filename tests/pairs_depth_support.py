"""What the GPU tests of the pairs batch's depth stages share (helper, no test in it): one call of refine / filter / search / smooth /
carry on a prepared object, held to the stage's numpy restatement run on entries rebuilt from the object's own device arrays
(pairs_oracle.read_entry).  The checks are those of tests/test_gpu_pairs_{refine,filter,search,smooth,carry}.py, which import them
from here, as do tests/test_gpu_pairs_depth_options.py and tests/test_gpu_pairs_depth_rounds.py.

Decisions on a knife edge (`knife`).  The device's pose prologue rounds the pose entries in another order than the host spline the
restatements use, so a quantity both compute can differ in its last bits.  Two decisions of steps 1 and 2 are discontinuous in such a
quantity: the truncation of a patch pixel, (int)(ox + dx), and the test of a tap against the image bounds.  A keypoint is on the
knife edge when the restated ox + dx or oy + dy of one of its pixels lies within MARGIN of an integer, or a restated tap coordinate
of a pixel inside the current image lies within MARGIN of 0, W - 1 or H - 1.  The mask comes from the restatement alone, never from
where the device disagrees.  Nothing else needs one: the clamp at max_rel_step and the bilinear blend at a whole coordinate are
continuous in what they clamp or blend, h_rho > 0 fails only for an exact zero, and no depth of these tests (1 .. 3, or the 0.005 of
a caller's bad point, moved by at most 25 %) comes near z_min = 0.01.  The filter's gate keeps its own rule (`filter_check`)."""
import numpy as np

import pairs_carry_ref as cref
import pairs_device as dv
import pairs_filter_ref as fref
import pairs_oracle as po
import pairs_refine_ref as ref
import pairs_search_ref as sref
import pairs_smooth_ref as mref

MARGIN = 1e-9     # pixels
MAX_SHARE = 0.01  # of a (pair, level)'s keypoints that may lie on a knife edge


def rel(got, want):
    """max |got - want| / max |want| over the finite entries of `want`; inf unless the others (NaN, +-inf: what an invalid depth
    leaves) are the same in both."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    if not fin.all():
        if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])):
            return float("inf")
        got, want = got[fin], want[fin]
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    diff = float(np.max(np.abs(got - want))) if want.size else 0.0
    return diff / scale if scale > 0 else diff


def changed(a, b):
    """Where two arrays of doubles hold other bits (a NaN that stays a NaN has not changed)."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64) != np.ascontiguousarray(b, np.float64).view(np.uint64)


def bits(a, b):
    """The same bits, NaN payloads aside."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and dv.same_bits(a[~nan], b[~nan])


def same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def level_layout(pb, level):
    """(entries per pair, first entry of each reported level, the reported levels) of the per-keypoint arrays."""
    cap = pb.capacities()
    if level < 0:
        return sum(cap), np.concatenate([[0], np.cumsum(cap)]).tolist(), list(range(pb.L))
    return cap[level], {level: 0}, [level]


def depths(pb):
    return [dv.peek(pb.array[e].d_kp_z, pb.array[e].K, np.float64) for e in range(pb.B * pb.L)]


# ---------------------------------------------------------------------------------------------------------------- the knife edge
def knife(e, pose_list, z=None, margin=MARGIN):
    """K bools from the restatement alone: the keypoints whose pixel truncation or tap test could fall the other way within
    `margin` pixels, at depths z (default: the entry's)."""
    z = np.asarray(e["z"] if z is None else z, np.float64)
    if e["K"] == 0:
        return np.zeros(0, bool)
    t, q = pose_list[e["S"] // 2]
    pat = e["pattern"].reshape(-1, 2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ox, oy = ref.patch_centres(t, q, e["xy"], z, e["intr"])
        cx, cy = ox[:, None] + pat[None, :, 0], oy[:, None] + pat[None, :, 1]
        whole = ((np.abs(cx - np.rint(cx)) <= margin) | (np.abs(cy - np.rint(cy)) <= margin)).any(1)
        return whole | (ref.keypoints(e, pose_list, z=z)["rim"] <= margin)


def knife_of(lib, capi, e, k, zs=None):
    """`knife` of an entry at its own depths, or over every column of zs (K x ND: the search's candidates); all False off the knots."""
    if not ref.on_knots(e, k):
        return np.zeros(e["K"], bool)
    pose_list = ref.poses(lib, capi, e, k)
    if zs is None:
        return knife(e, pose_list)
    out = np.zeros(e["K"], bool)
    for d in range(zs.shape[1]):
        out |= knife(e, pose_list, z=zs[:, d])
    return out


def _kept(mbavo, ctx, e, k, exclude, tag, b, l, zs=None):
    """The keypoints a comparison keeps: all without `exclude`, else those off the knife edge, whose share is asserted."""
    if not exclude:
        return np.ones(e["K"], bool)
    ex = knife_of(ctx.lib, mbavo.capi, e, k, zs)
    if ex.any():
        print("%s pair %d level %d: %d of %d keypoints on a knife edge, left out" % (tag, b, l, ex.sum(), e["K"]))
    assert ex.sum() <= MAX_SHARE * e["K"], (tag, b, l, int(ex.sum()), e["K"])
    return ~ex


# ---------------------------------------------------------------------------------------------------------------- refine
def refine_arrays(pb, level):
    import torch
    cap = pb.capacities()
    n = sum(cap) if level < 0 else cap[level]
    mk = lambda dt, fill: torch.full((pb.B, n), fill, dtype=dt, device="cuda:0")
    return dict(g=mk(torch.float64, -7.0), h=mk(torch.float64, -7.0), cost=mk(torch.float64, -7.0), valid=mk(torch.int32, -7)), cap


def refine_run(pb, level=0, apply=False, **kw):
    arr, cap = refine_arrays(pb, level)
    rc, out = pb.refine_depths(level=level, apply=apply, **arr, **kw)
    assert rc == 0, rc
    return out, {key: v.cpu().numpy() for key, v in arr.items()}, cap


def refine_check(mbavo, ctx, pb, counts, k, tag, bound, level=0, apply=False, exclude=False, log=None, **kw):
    """One call against the restatement; returns the largest relative difference.  exclude: leave the keypoints of `knife` out (the
    records, which sum over all keypoints, are then held only where no keypoint is left out).  log: a list that takes
    (tag, b, l, K, left out, largest relative difference, device arrays of the entry, restatement, entry)."""
    capi = mbavo.capi
    entries = {(b, l): po.read_entry(capi, pb.array[b * pb.L + l], k) for b in range(pb.B) for l in (range(pb.L) if level < 0 else [level])}
    out, arr, cap = refine_run(pb, level, apply, **kw)
    worst, off = 0.0, np.concatenate([[0], np.cumsum(cap)])
    for (b, l), e in entries.items():
        want = ref.refine(ctx.lib, capi, e, k, cap[l], **kw)
        keep = _kept(mbavo, ctx, e, k, exclude, tag, b, l)
        whole = bool(keep.all())
        r = out[b * pb.L + l] if level < 0 else out[b]
        K, o0 = e["K"], (off[l] if level < 0 else 0)
        assert K == counts[b, l] and (r.status, r.num_keypoints) == (0, K), (tag, b, l)
        if whole:
            assert (r.num_full, r.num_moved) == (want["num_full"], want["num_moved"]), (tag, b, l)
        assert np.array_equal(arr["valid"][b, o0:o0 + K][keep], want["valid"][keep]), (tag, b, l)
        for key in ("g", "h", "cost", "valid"):
            assert (arr[key][b, o0 + K:(off[l + 1] if level < 0 else cap[level])] == -7).all(), (tag, b, l, key)  # entries from K on: not written
        rels = {key: rel(arr[key][b, o0:o0 + K][keep], want[key][keep]) for key in ("g", "h", "cost")}
        if whole:
            rels["rec_cost"] = abs(r.cost - want["sum_cost"]) / max(abs(want["sum_cost"]), 1e-300)
            rels["rec_rel"] = abs(r.sum_sq_rel - want["sum_sq_rel"]) / max(abs(want["sum_sq_rel"]), 1e-300) if want["num_moved"] else abs(r.sum_sq_rel)
        z_now = dv.peek(pb.array[b * pb.L + l].d_kp_z, K, np.float64)
        if apply:
            rels["z"] = rel(z_now[keep], want["z_new"][keep])
            assert np.array_equal(changed(z_now, e["z"])[keep], (want["moved"] & changed(want["z_new"], e["z"]))[keep]), (tag, b, l)
        else:
            assert dv.same_bits(z_now, e["z"]), (tag, b, l)
        print("%s pair %d level %d K %d full %d moved %d: %s" % (tag, b, l, K, r.num_full, r.num_moved, "  ".join("%s %.3g" % kv for kv in rels.items())))
        assert all(v <= bound for v in rels.values()), (tag, b, l, rels, bound)
        worst = max([worst] + list(rels.values()))
        if log is not None:
            log.append((tag, b, l, K, int((~keep).sum()), max(rels.values()), {key: arr[key][b, o0:o0 + K] for key in arr}, want, e))
    return worst


# ---------------------------------------------------------------------------------------------------------------- filter
def filter_state(pb):
    """The filter state read back: dict of B x stride arrays, and the level offsets."""
    s = pb.filter_state()
    n = pb.B * sum(pb.capacities())
    out = {key: dv.peek(s["ptr"][i], n, dt).reshape(pb.B, -1) for i, (key, dt) in enumerate((("mu", np.float64), ("info", np.float64),
                                                                                            ("n_obs", np.int32), ("n_rej", np.int32)))}
    return out, s["offset"]


def filter_slot(st, off, b, l, K):
    return {key: v[b, off[l]:off[l] + K].copy() for key, v in st.items()}


def filter_run(pb, **kw):
    rc, out = pb.filter_depths(**kw)
    assert rc == 0, rc
    return out


def filter_check(mbavo, ctx, pb, k, tag, seeded, bound, first=False, level=-1, apply=True, exclude=False, log=None, **opts):
    """One call against the restatement fed the entries and the state as they are before it.  seeded[b][l]: what the call must
    seed.  A fused / rejected decision may differ on a keypoint whose c2 lies within `bound` (relative) of the gate; such a keypoint
    is left out, at most 1 % of an entry's.  exclude: `knife`'s keypoints are left out as well.  Returns (largest relative
    difference, records)."""
    capi = mbavo.capi
    levels = range(pb.L) if level < 0 else [level]
    cap = pb.capacities()
    entries = {(b, l): po.read_entry(capi, pb.array[b * pb.L + l], k) for b in range(pb.B) for l in levels}
    if first:
        before, off = None, np.concatenate([[0], np.cumsum(cap)])
    else:
        before, off = filter_state(pb)
    out = filter_run(pb, level=level, apply=apply, **opts)
    after, off = filter_state(pb)
    worst, gate = 0.0, opts.get("gate_chi2", 0.0)
    for (b, l), e in entries.items():
        K = e["K"]
        st0 = fref.empty_state(K) if before is None else filter_slot(before, off, b, l, K)
        want = fref.filter(ctx.lib, capi, e, k, cap[l], st0, seeded[b][l], **opts)
        for s in (1.0 - bound, 1.0 + bound):  # the gate has room: the restatement decides alike with g moved by the bound
            moved = fref.filter(ctx.lib, capi, e, k, cap[l], st0, seeded[b][l], g_scale=s, **opts)
            assert np.array_equal(moved["fused"], want["fused"]) and np.array_equal(moved["rejected"], want["rejected"]), (tag, b, l)
        off_edge = _kept(mbavo, ctx, e, k, exclude, tag, b, l)
        r = out[b * pb.L + l] if level < 0 else out[b]
        got = filter_slot(after, off, b, l, K)
        base = fref.seed(e["z"], opts.get("prior_rel_sigma", 0.0)) if seeded[b][l] else st0
        d_fused, d_rej = got["n_obs"] - base["n_obs"], got["n_rej"] - base["n_rej"]
        differ = ((d_fused != want["fused"]) | (d_rej != want["rejected"])) & off_edge
        if differ.any():
            near = np.abs(want["c2"] / gate - 1.0) <= bound
            print("%s pair %d level %d: %d decisions differ, %d of them at the gate" % (tag, b, l, differ.sum(), (differ & near).sum()))
            assert not (differ & ~near).any() and differ.sum() <= 0.01 * K, (tag, b, l)
        keep = ~differ & off_edge
        whole = bool(keep.all())
        assert (r.status, r.num_keypoints, r.seeded) == (0, K, int(seeded[b][l])), (tag, b, l)
        if off_edge.all():
            assert r.num_full == want["num_full"], (tag, b, l)
        if whole:
            assert (r.num_fused, r.num_rejected) == (want["num_fused"], want["num_rejected"]), (tag, b, l)
        for key in after:  # entries from K on: never written
            tail = after[key][b, off[l] + K:off[l] + cap[l]]
            assert first or np.array_equal(tail, before[key][b, off[l] + K:off[l] + cap[l]]), (tag, b, l, key)
            assert not first or (tail == 0).all(), (tag, b, l, key)
        rels = {key: rel(got[key][keep], want["state"][key][keep]) for key in ("mu", "info")}
        z_now = dv.peek(pb.array[b * pb.L + l].d_kp_z, K, np.float64)
        rels["z"] = rel(z_now[keep], (want["z_new"] if apply else e["z"])[keep])
        if not apply:
            assert dv.same_bits(z_now, e["z"]), (tag, b, l)
        if off_edge.all():
            rels["rec_cost"] = abs(r.cost - want["sum_cost"]) / max(abs(want["sum_cost"]), 1e-300)
        if whole:
            for key in ("sum_info", "sum_sq_rel"):
                rels[key] = abs(getattr(r, key) - want[key]) / max(abs(want[key]), 1e-300) if want["num_fused"] else abs(getattr(r, key))
        print("%s pair %d level %d K %d full %d fused %d rejected %d seeded %d: %s" % (tag, b, l, K, r.num_full, r.num_fused, r.num_rejected, r.seeded,
                                                                                  "  ".join("%s %.3g" % kv for kv in rels.items())))
        assert all(v <= bound for v in rels.values()), (tag, b, l, rels, bound)
        worst = max([worst] + list(rels.values()))
        if log is not None:
            log.append((tag, b, l, K, int((~keep).sum()), max(rels.values())))
    return worst, out


# ---------------------------------------------------------------------------------------------------------------- search
def search_run(pb, nd, lo, hi, level=-1, **kw):
    """One call with every array: (records, dict of host arrays B x n (volume B x n x nd))."""
    import torch
    n, off, levels = level_layout(pb, level)
    mk = lambda dt, m: torch.full((pb.B, n * m), -7, dtype=dt, device="cuda:0")
    t = dict(rho=mk(torch.float64, 1), cost_best=mk(torch.float64, 1), cost_second=mk(torch.float64, 1), curv=mk(torch.float64, 1),
             best=mk(torch.int32, 1), num_full=mk(torch.int32, 1), volume=mk(torch.float64, nd))
    rc, out = pb.search_depths(nd, lo, hi, level=level, **t, **kw)
    assert rc == 0, rc
    arr = {key: v.cpu().numpy() for key, v in t.items()}
    arr["volume"] = arr["volume"].reshape(pb.B, n, nd)
    return out, arr


def search_check_selection(pb, out, arr, nd, lo, hi, level=-1, relative=0, z=None, tag="", **opts):
    """Arrays and records of one call against the numpy selection applied to the device's own volume, bit for bit.  z: the depths
    before the call.  Returns per (b, l) the restatement's (selection, accepted, z_new)."""
    n, off, levels = level_layout(pb, level)
    cap = pb.capacities()
    res = {}
    for b in range(pb.B):
        for i, l in enumerate(levels):
            e = b * pb.L + l
            K, P = pb.array[e].K, pb.array[e].P
            o0 = off[l]
            zz = z[e]
            lo_k, step, rho, D = sref.candidates(zz, nd, lo, hi, relative)
            vol = arr["volume"][b, o0:o0 + K]
            sel = sref.select(vol, lo_k, step)
            for key in ("rho", "cost_best", "cost_second", "curv", "best", "num_full"):
                got = arr[key][b, o0:o0 + K]
                if got.dtype == np.float64:  # (NaN payloads aside, the same bits)
                    fin = ~np.isnan(got)
                    assert np.array_equal(fin, ~np.isnan(sel[key])) and dv.same_bits(got[fin], sel[key][fin]), (tag, b, l, key)
                else:
                    assert np.array_equal(got, sel[key]), (tag, b, l, key)
                assert (arr[key][b, o0 + K:o0 + cap[l]] == -7).all(), (tag, b, l, key)  # entries from K on: not written
            assert (arr["volume"][b, o0 + K:o0 + cap[l]] == -7).all(), (tag, b, l)
            acc, z_new, ratio = sref.accept(sel, **opts)
            want = sref.records(sel, acc, ratio, P, cap[l])
            r = out[b * len(levels) + i]
            assert (r.status, r.num_keypoints, r.num_searched, r.num_accepted) == (0, K, want["num_searched"], want["num_accepted"]), (tag, b, l)
            assert np.float64(r.cost).tobytes() == np.float64(want["cost"]).tobytes(), (tag, b, l, r.cost, want["cost"])
            assert np.float64(r.sum_ratio).tobytes() == np.float64(want["sum_ratio"]).tobytes(), (tag, b, l, r.sum_ratio, want["sum_ratio"])
            res[(b, l)] = (dict(sel, volume=vol, step=step, rho_best=lo_k + sel["best"].astype(np.float64) * step), acc, z_new)
    return res


def search_check_volume(mbavo, ctx, pb, k, entries, arr, nd, lo, hi, bound, level=-1, relative=0, tag="", exclude=True, log=None):
    """The device's volume against pairs_search_ref.volume on the entries read before the call: which candidates are full, exactly,
    and the costs within `bound` of the largest, keypoints on a knife edge at any candidate depth left out.  Returns the largest
    relative difference."""
    n, off, levels = level_layout(pb, level)
    worst = 0.0
    for b in range(pb.B):
        for l in levels:
            e = entries[(b, l)]
            K = e["K"]
            lo_k, step, rho, D = sref.candidates(e["z"], nd, lo, hi, relative)
            want = sref.volume(e, ref.poses(ctx.lib, mbavo.capi, e, k), D)
            keep = _kept(mbavo, ctx, e, k, exclude, tag, b, l, zs=D)
            got = arr["volume"][b, off[l]:off[l] + K][keep]
            want = want[keep]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, b, l)
            fin = ~np.isnan(want)
            r = rel(got[fin], want[fin])
            print("%s pair %d level %d K %d: volume %.3g over %d full candidates" % (tag, b, l, K, r, fin.sum()))
            assert r <= bound, (tag, b, l, r, bound)
            worst = max(worst, r)
            if log is not None:
                log.append((tag, b, l, K, int((~keep).sum()), r))
    return worst


# ---------------------------------------------------------------------------------------------------------------- smooth
def smooth_entry(pb, b, l):
    q = pb.array[b * pb.L + l]
    xy = dv.peek(q.d_kp_xy, 2 * q.K, np.float64).reshape(-1, 2)
    z = dv.peek(q.d_kp_z, q.K, np.float64)
    img = dv.peek(q.d_ref_img, q.H * q.W, np.uint8).reshape(q.H, q.W)
    I = img[xy[:, 1].astype(int), xy[:, 0].astype(int)] if q.K else np.zeros(0, np.uint8)
    return xy, z, I


def smooth_run(pb, level=-1, weight=None, **kw):
    import torch
    n, off, levels = level_layout(pb, level)
    t = dict(rho=torch.full((pb.B, n), -7.0, dtype=torch.float64, device="cuda:0"), flags=torch.full((pb.B, n), 77, dtype=torch.uint8, device="cuda:0"),
             support=torch.full((pb.B, n), -7, dtype=torch.int32, device="cuda:0"))
    rc, out = pb.smooth_depths(level=level, weight=weight, **t, **kw)
    assert rc == 0, rc
    return out, {key: v.cpu().numpy() for key, v in t.items()}


def smooth_check(pb, level=-1, weights_of=None, tag="", **kw):
    """One call against the restatement on what the object held before it; returns (records, arrays, restatements)."""
    n, off, levels = level_layout(pb, level)
    cap = pb.capacities()
    before = {(b, l): smooth_entry(pb, b, l) for b in range(pb.B) for l in levels}
    weight = None
    if weights_of is not None and kw.get("weights") == 2:
        weight = dv.dev(weights_of)[0]
    out, arr = smooth_run(pb, level=level, weight=weight, **kw)
    ref_kw = {k: v for k, v in kw.items() if k not in ("apply", "sync_filter", "weights")}
    res = {}
    for b in range(pb.B):
        for i, l in enumerate(levels):
            xy, z, I = before[(b, l)]
            K, o0 = len(z), off[l]
            w = None
            if kw.get("weights") == 2:
                w = weights_of[b, o0:o0 + K]
            elif kw.get("weights") == 1:
                w = weights_of[b, sum(cap[:l]):sum(cap[:l]) + K]
            m = mref.smooth(xy, z, weights=w, I=I, **ref_kw)
            r = out[b * len(levels) + i]
            assert np.array_equal(arr["flags"][b, o0:o0 + K], m["flags"]) and np.array_equal(arr["support"][b, o0:o0 + K], m["support"]), (tag, b, l)
            assert bits(arr["rho"][b, o0:o0 + K], m["rho"]), (tag, b, l)
            assert (arr["flags"][b, o0 + K:o0 + cap[l]] == 77).all() and (arr["rho"][b, o0 + K:o0 + cap[l]] == -7).all(), (tag, b, l)  # from K on
            got = (r.num_keypoints, r.num_valid, r.num_supported, r.num_filled, r.num_outliers, r.num_moved, r.sum_support)
            want = tuple(m[key] for key in ("num_keypoints", "num_valid", "num_supported", "num_filled", "num_outliers", "num_moved", "sum_support"))
            assert got == want, (tag, b, l, got, want)
            assert abs(r.sum_sq_rel - m["sum_sq_rel"]) <= max(K, 1) * 2.0 ** -52 * m["sum_sq_rel"], (tag, b, l, r.sum_sq_rel, m["sum_sq_rel"])
            z_after = smooth_entry(pb, b, l)[1]
            assert bits(z_after, m["z_new"] if kw.get("apply") else z), (tag, b, l, "depths")
            res[(b, l)] = m
    return out, arr, res


# ---------------------------------------------------------------------------------------------------------------- carry
def carry_entry(pb, b, l):
    q = pb.array[b * pb.L + l]
    return dv.peek(q.d_kp_xy, 2 * q.K, np.float64).reshape(-1, 2), dv.peek(q.d_kp_z, q.K, np.float64), q.H, q.W


def carry_save_check(pb, listed, Ts, info=None, tag="", intr_of=None, **kw):
    """carry_save against the restatement on what the object holds; returns (records, {(b, l): restatement}).  intr_of: None (the
    object's one camera) or pair -> the level-0 intrinsics of the pair's camera."""
    cap = pb.capacities()
    rc, out = pb.carry_save(listed, Ts, **kw)
    assert rc == 0, (tag, rc)
    res = {}
    for i, b in enumerate(listed):
        for l in range(pb.L):
            xy, z, h, w = carry_entry(pb, b, l)
            o0 = sum(cap[:l])
            wts = None if not kw.get("weights") else info[b, o0:o0 + len(z)]
            s = cref.save(xy, z, cref.level_intrinsics(pb.intr if intr_of is None else intr_of(b), l), w, h, Ts[i], deflate=kw.get("deflate", 1.0), w=wts,
                          z_min=kw.get("z_min", 0.0), z_max=kw.get("z_max", 0.0), cap=cap[l])
            r = out[i * pb.L + l]
            got, want = (r.num_keypoints, r.num_valid, r.num_carried), (s["num_keypoints"], s["num_valid"], s["num_carried"])
            print("%s save pair %d level %d: K %d valid %d carried %d sum_w %.17g (restated %.17g)" % (tag, b, l, *got, r.sum_w, s["sum_w"]))
            assert got == want and same(r.sum_w, s["sum_w"]), (tag, b, l, got, want, r.sum_w, s["sum_w"])
            res[(b, l)] = s
    return out, res


def carry_arrays(pb):
    import torch
    n = sum(pb.capacities())
    return dict(rho=torch.full((pb.B, n), -7.0, dtype=torch.float64, device="cuda:0"), info=torch.full((pb.B, n), -7.0, dtype=torch.float64, device="cuda:0"),
                count=torch.full((pb.B, n), -7, dtype=torch.int32, device="cuda:0"), flags=torch.full((pb.B, n), 77, dtype=torch.uint8, device="cuda:0"))


def carry_adopt_check(pb, listed, saved, radius, tag="", **kw):
    """carry_adopt against the restatement; returns (records, arrays, {(b, l): restatement})."""
    cap = pb.capacities()
    before = {(b, l): carry_entry(pb, b, l) for b in range(pb.B) for l in range(pb.L)}
    t = carry_arrays(pb)
    rc, out = pb.carry_adopt(listed, **t, **kw)
    assert rc == 0, (tag, rc)
    arr = {k: v.cpu().numpy() for k, v in t.items()}
    ref_kw = {k: v for k, v in kw.items() if k not in ("apply", "seed_filter")}
    res = {}
    for b in range(pb.B):
        for l in range(pb.L):
            xy, z, _, _ = before[(b, l)]
            K, o0 = len(z), sum(cap[:l])
            z_after = carry_entry(pb, b, l)[1]
            if b not in listed:  # an unlisted pair keeps its bytes
                assert (arr["flags"][b] == 77).all() and (arr["rho"][b] == -7).all() and (arr["count"][b] == -7).all() and (arr["info"][b] == -7).all()
                assert bits(z_after, z), (tag, b, l)
                continue
            m = cref.adopt(xy, z, saved[(b, l)], radius, cap=cap[l], **ref_kw)
            r = out[listed.index(b) * pb.L + l]
            assert np.array_equal(arr["flags"][b, o0:o0 + K], m["flags"]) and np.array_equal(arr["count"][b, o0:o0 + K], m["count"]), (tag, b, l)
            assert bits(arr["rho"][b, o0:o0 + K], m["rho"]) and bits(arr["info"][b, o0:o0 + K], m["info"]), (tag, b, l)
            assert (arr["flags"][b, o0 + K:o0 + cap[l]] == 77).all() and (arr["rho"][b, o0 + K:o0 + cap[l]] == -7).all(), (tag, b, l)  # from K on
            got, want = (r.num_keypoints, r.num_adopted, r.num_empty), (m["num_keypoints"], m["num_adopted"], m["num_empty"])
            print("%s adopt pair %d level %d: K %d adopted %d empty %d sum_info %.17g sum_sq_rel %.17g" % (tag, b, l, *got, r.sum_info, r.sum_sq_rel))
            assert got == want and same(r.sum_info, m["sum_info"]) and same(r.sum_sq_rel, m["sum_sq_rel"]), (tag, b, l, got, want)
            assert bits(z_after, m["z_new"] if kw.get("apply") else z), (tag, b, l, "depths")
            res[(b, l)] = m
    return out, arr, res
