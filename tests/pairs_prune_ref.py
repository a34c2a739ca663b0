"""numpy restatement of mbavo_pairs_prune_keypoints (include/mbavo.h, steps 1 - 5) on one (pair, level) (helper, no test in it): the
verdict of every keypoint under the first criterion that holds, the counts, min_keep, the stable compaction of the coordinates, the
depths and the filter's four state arrays, and the tail left as it was.  Arrays come at their full capacity, so that the entries
from the new count on can be compared with what they held.  Below it: the options struct, the raw call, and what the GPU tests share --
a snapshot of everything a prune may touch, read through the problems' device pointers, and one call held to the restatement."""
import ctypes as C

import numpy as np

KEEP, BY_FLAG, BY_DEPTH, BY_FILTER = 0, 1, 2, 3
STATE_KEYS = (("mu", np.float64), ("info", np.float64), ("n_obs", np.int32), ("n_rej", np.int32))
CRITERIA = ("drop_mask", "use_filter", "min_info", "min_obs", "rej_limit", "check_depth", "z_min", "z_max")


def verdicts(K, flags=None, drop_mask=0, z=None, check_depth=0, z_min=0.0, z_max=0.0, state=None, use_filter=0, min_info=0.0, min_obs=0, rej_limit=0):
    """Step 1: K ints, KEEP or the FIRST criterion that holds -- flag, depth, filter, in this order."""
    v = np.zeros(K, np.int64)
    if flags is not None and drop_mask != 0:
        f = np.asarray(flags[:K], np.uint8).astype(np.int64)
        hit = (f < 32) & (((int(drop_mask) >> np.minimum(f, 31)) & 1) == 1)
        v[hit] = BY_FLAG
    if check_depth:
        z_min = 1e-2 if z_min == 0 else z_min
        D = np.asarray(z[:K], np.float64)
        with np.errstate(invalid="ignore"):
            inside = np.isfinite(D) & (D >= z_min) & ((z_max == 0) | (D <= z_max))
        v[(v == KEEP) & ~inside] = BY_DEPTH
    if use_filter:
        with np.errstate(invalid="ignore"):
            bad = np.zeros(K, bool)
            if min_info > 0:
                bad |= state["info"][:K] < min_info  # (a NaN info does not drop)
            if min_obs > 0:
                bad |= state["n_obs"][:K] < min_obs
            if rej_limit > 0:
                bad |= state["n_rej"][:K] >= rej_limit
        v[(v == KEEP) & bad] = BY_FILTER
    return v


def prune(K, xy, z, state=None, flags=None, apply=1, min_keep=0, **crit):
    """The whole call on one (pair, level) that holds K keypoints in arrays of its capacity: xy cap x 2, z cap, state None (the
    filter's state does not exist) or dict(mu, info, n_obs, n_rej) of cap entries each, flags None or at least K bytes.  Returns
    dict(K (after), xy, z, state (copies, as the call leaves them), keep (K bytes as d_keep receives them), record (status,
    num_before, num_kept, by_flag, by_depth, by_filter, skipped, pad))."""
    assert set(crit) <= set(CRITERIA), crit
    xy, z = np.array(xy, np.float64).reshape(-1, 2), np.array(z, np.float64)
    state = None if state is None else {key: np.array(state[key], dt) for key, dt in STATE_KEYS}
    v = verdicts(K, flags=flags, z=z, state=state, **crit)
    stays = v == KEEP
    kept = int(stays.sum())
    skipped = kept < K and kept < min_keep
    if skipped:
        stays = np.ones(K, bool)
    K_new = K
    if apply and not skipped:
        src = np.flatnonzero(stays)  # ascending: survivor i goes to its rank among the survivors
        xy[:kept], z[:kept] = xy[src], z[src]
        if state is not None:
            for key in state:
                state[key][:kept] = state[key][src]
        K_new = kept
    record = (0, K, K if skipped else kept, int((v == BY_FLAG).sum()), int((v == BY_DEPTH).sum()), int((v == BY_FILTER).sum()), int(skipped), 0)
    return dict(K=K_new, xy=xy, z=z, state=state, keep=stays.astype(np.uint8), record=record, verdicts=v)


def opts_struct(capi, level=-1, apply=0, min_keep=0, **crit):
    assert set(crit) <= set(CRITERIA), crit
    o = capi.PairsPruneOpts()
    o.level, o.apply, o.min_keep = level, apply, min_keep
    for key, val in crit.items():
        setattr(o, key, val)
    return o


def call(lib, handle, pairs, o, flags=None, out=None, keep=None):
    """The raw entry point: pairs None (n = 0, every pair) or a list; optional ctypes records and device pointers (ints)."""
    keys = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    return lib.mbavo_pairs_prune_keypoints(handle, 0 if keys is None else int(keys.size), None if keys is None else keys.ctypes.data_as(C.POINTER(C.c_int)),
                                           None if o is None else C.byref(o), flags, out, keep)


def record_tuple(r):
    return (r.status, r.num_before, r.num_kept, r.by_flag, r.by_depth, r.by_filter, r.skipped, r.pad)


# ------------------------------------------------------------------------------------------------------------ on the device
def layout(pb, level):
    """(entries per pair, {level: first entry}, the reported levels) of the caller's byte arrays of a call on `level`."""
    cap = pb.capacities()
    if level < 0:
        return sum(cap), {l: sum(cap[:l]) for l in range(pb.L)}, list(range(pb.L))
    return cap[level], {level: 0}, [level]


def device_counts(pb):
    """The device's B x L counts, as a count-only call without criteria reports them (num_before), nothing changed."""
    rc, out = pb.prune_keypoints(level=-1, apply=False)
    assert rc == 0, rc
    return np.array([r.num_before for r in out], np.int32).reshape(pb.B, pb.L)


def snapshot(pb):
    """Everything a prune may touch: per (pair, level) K of mbavo_pairs_problems and the keypoint arrays at their full capacity, read
    through the problems' device pointers; the filter's state whole (None before its first call)."""
    import pairs_device as dv
    cap = pb.capacities()
    ents = {}
    for b in range(pb.B):
        for l in range(pb.L):
            q = pb.array[b * pb.L + l]
            ents[(b, l)] = dict(K=int(q.K), xy=dv.peek(q.d_kp_xy, 2 * cap[l], np.float64).reshape(-1, 2), z=dv.peek(q.d_kp_z, cap[l], np.float64))
    try:
        s = pb.filter_state()
    except RuntimeError:
        return dict(ents=ents, state=None)
    n = pb.B * sum(cap)
    state = {key: dv.peek(s["ptr"][i], n, dt).reshape(pb.B, -1) for i, (key, dt) in enumerate(STATE_KEYS)}
    return dict(ents=ents, state=state)


def slot(snap, pb, b, l):
    """The state entries of a (pair, level) at its capacity, or None."""
    if snap["state"] is None:
        return None
    cap = pb.capacities()
    o = sum(cap[:l])
    return {key: v[b, o:o + cap[l]] for key, v in snap["state"].items()}


def same_entry(pb, x, y, b, l):
    """A (pair, level) of two snapshots holds the same bits and the same K."""
    import pairs_device as dv
    ex, ey = x["ents"][(b, l)], y["ents"][(b, l)]
    ok = ex["K"] == ey["K"] and dv.same_bits(ex["xy"], ey["xy"]) and dv.same_bits(ex["z"], ey["z"])
    sx, sy = slot(x, pb, b, l), slot(y, pb, b, l)
    if (sx is None) != (sy is None):
        return False
    return ok and (sx is None or all(dv.same_bits(np.ascontiguousarray(sx[key]), np.ascontiguousarray(sy[key])) for key in sx))


def unchanged(pb, x, y):
    return all(same_entry(pb, x, y, b, l) for b in range(pb.B) for l in range(pb.L))


def run_and_check(pb, listed=None, level=-1, apply=True, flags=None, min_keep=0, tag="", **crit):
    """One call with records and keep bytes against the restatement on what the object held before it, bit for bit: keypoint arrays
    and state at their full capacity (so the tail too), K of mbavo_pairs_problems, the device's counts, the records, d_keep; pairs
    not listed and levels not reported keep their bits.  flags: None or a host array in the call's layout.  Returns (records, the
    restatements per served (pair, level), the snapshot after)."""
    import torch
    import pairs_device as dv
    n, off, levels = layout(pb, level)
    cap = pb.capacities()
    pairs = list(range(pb.B)) if listed is None else list(listed)
    before = snapshot(pb)
    f_dev = None if flags is None else dv.dev(np.ascontiguousarray(flags, np.uint8))[0]
    keep = torch.full((pb.B, n), 99, dtype=torch.uint8, device="cuda:0")
    rc, out = pb.prune_keypoints(listed, level=level, apply=apply, flags=f_dev, keep=keep, min_keep=min_keep, **crit)
    assert rc == 0, (tag, rc)
    stats = pb.prune_stats()
    after = snapshot(pb)
    keep = keep.cpu().numpy()
    counts = device_counts(pb)
    res = {}
    for b in range(pb.B):
        for l in range(pb.L):
            e0 = before["ents"][(b, l)]
            if b not in pairs or l not in levels:
                assert same_entry(pb, before, after, b, l) and counts[b, l] == e0["K"], (tag, b, l, "not served, changed")
                if l in levels:
                    assert (keep[b, off[l]:off[l] + cap[l]] == 99).all(), (tag, b, l, "keep bytes of a pair not listed")
                continue
            fl = None if flags is None else np.asarray(flags).reshape(pb.B, n)[b, off[l]:off[l] + cap[l]]
            want = prune(e0["K"], e0["xy"], e0["z"], slot(before, pb, b, l), flags=fl, apply=apply, min_keep=min_keep, **crit)
            e1 = after["ents"][(b, l)]
            r = out[pairs.index(b) * len(levels) + levels.index(l)]
            assert record_tuple(r) == want["record"], (tag, b, l, record_tuple(r), want["record"])
            assert e1["K"] == want["K"] == counts[b, l], (tag, b, l, e1["K"], want["K"], counts[b, l])
            assert dv.same_bits(e1["xy"], want["xy"]) and dv.same_bits(e1["z"], want["z"]), (tag, b, l, "keypoints")
            s1 = slot(after, pb, b, l)
            if s1 is not None:
                for key in s1:
                    assert dv.same_bits(np.ascontiguousarray(s1[key]), want["state"][key]), (tag, b, l, key)
            assert np.array_equal(keep[b, off[l]:off[l] + e0["K"]], want["keep"]), (tag, b, l, "keep")
            assert (keep[b, off[l] + e0["K"]:off[l] + cap[l]] == 99).all(), (tag, b, l, "keep bytes from K on")
            res[(b, l)] = want
    return out, res, after, stats
