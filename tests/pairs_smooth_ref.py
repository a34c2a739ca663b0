"""numpy restatement of mbavo_pairs_smooth_depths (include/mbavo.h, steps 1 - 8) on one (pair, level) (helper, no test in it): a
brute-force O(K^2) neighbour search -- no bins, so nothing of the device's index is restated; `smooth` takes its rows in blocks
(`neighbour_rows`, the predicate of `neighbours`) -- and the sums of step 3 formed
keypoint by keypoint over ascending j, each product rounded, added left to right.  float64, operation by operation as the header
writes them."""
import ctypes as C

import numpy as np

import pairs_filter_scene as fs
import pairs_refine_scene as sc
import pairs_search_ref as sref

# the setting of the property tests (tests/test_pairs_smooth_api.py says where it comes from)
SWEEP = dict(radius=6, min_support=3, max_rel_diff=0.125, strength=1.0, fill=1)
INVALID, SUPPORTED, FILLED, OUTLIER = 0, 1, 2, 3


def clean_weights(w):
    """Step 1: a weight <= 0 or NaN counts as 0."""
    w = np.asarray(w, np.float64)
    return np.where(w > 0, w, 0.0)


def neighbours(xy, valid, w, I, radius, max_intensity_diff=0):
    """Step 2: K x K bool, [i, j] true iff j is in N_i."""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    K = len(xy)
    n = (np.abs(xy[:, None, 0] - xy[None, :, 0]) <= radius) & (np.abs(xy[:, None, 1] - xy[None, :, 1]) <= radius)
    n &= ~np.eye(K, dtype=bool)
    n &= (valid & (w > 0))[None, :]
    if max_intensity_diff != 0:
        I = np.asarray(I, np.int32)
        n &= np.abs(I[:, None] - I[None, :]) <= max_intensity_diff
    return n


def neighbour_rows(xy, valid, w, I, radius, max_intensity_diff=0, i0=0, i1=None):
    """Rows i0 .. i1 - 1 of `neighbours`: the same predicate on a block of rows, (i1 - i0) x K bool."""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    K = len(xy)
    i1 = K if i1 is None else min(i1, K)
    rows = np.arange(i0, i1)
    n = (np.abs(xy[i0:i1, None, 0] - xy[None, :, 0]) <= radius) & (np.abs(xy[i0:i1, None, 1] - xy[None, :, 1]) <= radius)
    n[rows - i0, rows] = False
    n &= (valid & (w > 0))[None, :]
    if max_intensity_diff != 0:
        I = np.asarray(I, np.int32)
        n &= np.abs(I[i0:i1, None] - I[None, :]) <= max_intensity_diff
    return n


BLOCK_CELLS = 1 << 24  # the most cells of the neighbour predicate `smooth` holds at a time


def _sum(values):
    """From 0.0, left to right (np.sum adds pairwise: not this)."""
    acc = np.float64(0.0)
    for v in values:
        acc = acc + v
    return acc


def smooth(xy, z, radius, min_support=1, max_rel_diff=0.1, strength=1.0, fill=0, weights=None, I=None, max_intensity_diff=0, z_min=0.0, z_max=0.0,
           order=None):
    """The whole call on one (pair, level): xy K x 2 whole pixels, z the depths before the call, weights None (ones) or K doubles, I
    the keyframe's bytes at the keypoints (needed with max_intensity_diff != 0).  `order`: None, or a function that reorders each
    keypoint's ascending neighbour list before the sums (the tests use it to show that the order matters).  Returns dict(rho, flags,
    support, z_new (the depths after apply = 1), moved, stands, and the record's fields)."""
    z = np.asarray(z, np.float64)
    K = z.size
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z_min = 1e-2 if z_min == 0 else z_min
    w = np.ones(K) if weights is None else clean_weights(weights)
    valid = np.isfinite(z) & (z > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho_all = 1.0 / z
    block = max(1, BLOCK_CELLS // max(K, 1))  # rows taken in blocks: K x K cells at once are gigabytes at K = 17000
    nb, nb0 = None, 0
    rho = np.full(K, np.nan)
    flags, support = np.zeros(K, np.uint8), np.zeros(K, np.int32)
    stands, moved = np.zeros(K, bool), np.zeros(K, bool)
    z_new = z.copy()
    rel2 = np.zeros(K)
    lam = np.float64(strength)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in np.flatnonzero(valid):
            ri, wi = rho_all[i], w[i]
            if nb is None or i >= nb0 + len(nb):
                nb0 = i
                nb = neighbour_rows(xy, valid, w, I, radius, max_intensity_diff, nb0, nb0 + block)
            js = np.flatnonzero(nb[i - nb0])
            if order is not None:
                js = order(js)
            agree = np.abs(rho_all[js] - ri) <= np.float64(max_rel_diff) * ri
            jc = js[agree]
            support[i] = jc.size
            proposal = None
            if jc.size >= min_support:
                flags[i] = SUPPORTED
                SW, SR = _sum(w[jc]), _sum(w[jc] * rho_all[jc])
                proposal = (wi * ri + lam * SR) / (wi + lam * SW)
            elif fill == 1 and js.size >= min_support:
                flags[i] = FILLED
                proposal = _sum(w[js] * rho_all[js]) / _sum(w[js])
            else:
                flags[i] = OUTLIER
            rho[i] = ri
            if proposal is not None:
                D = np.float64(1.0) / proposal
                if np.isfinite(D) and D >= z_min and (z_max == 0 or D <= z_max):
                    stands[i], rho[i], z_new[i] = True, proposal, D
                    moved[i] = proposal != ri
            rel = (rho[i] - ri) / ri
            rel2[i] = rel * rel
    return dict(rho=rho, flags=flags, support=support, z_new=z_new, stands=stands, moved=moved, rel2=rel2,
                num_keypoints=K, num_valid=int(valid.sum()), num_supported=int((flags == SUPPORTED).sum()), num_filled=int((flags == FILLED).sum()),
                num_outliers=int((flags == OUTLIER).sum()), num_moved=int(moved.sum()), sum_support=int(support[valid].sum()),
                sum_sq_rel=float(_sum(rel2[valid])))


def opts_struct(capi, radius=2, min_support=1, max_rel_diff=0.1, strength=1.0, level=-1, apply=0, fill=0, sync_filter=0, weights=0, max_intensity_diff=0,
                z_min=0.0, z_max=0.0):
    o = capi.PairsSmoothOpts()
    o.level, o.apply, o.fill, o.sync_filter, o.weights = level, apply, fill, sync_filter, weights
    o.radius, o.min_support, o.max_intensity_diff = radius, min_support, max_intensity_diff
    o.max_rel_diff, o.strength, o.z_min, o.z_max = max_rel_diff, strength, z_min, z_max
    return o


def call(lib, handle, o, out=None, weight=None, rho=None, flags=None, support=None):
    """The raw entry point with optional ctypes records and device pointers (ints)."""
    return lib.mbavo_pairs_smooth_depths(handle, None if o is None else C.byref(o), out, weight, rho, flags, support)


def noisy_search(lib, capi, b):
    """Pair b after the numpy search of tests/test_pairs_search_api.py's noise setting: (entry, truth, search result)."""
    e = sc.entry(b)
    e["curs"] = [np.ascontiguousarray(fs.frames(b, noise=fs.NOISE)[fs.T - 1])]
    e["cap"] = np.array([fs.caps(b)[fs.T - 1]])
    truth = e["z"].copy()
    return e, truth, sref.search(lib, capi, e, e["k"], e["K"], 9, 0.5, 1.5, 1)


def figures(z, truth, s):
    """(accepted keypoints more than one candidate step off, median relative depth error over the accepted)."""
    acc = s["accepted"]
    off = np.abs(1.0 / z[acc] - 1.0 / truth[acc]) / s["step"][acc]
    return int((off > 1.0).sum()), float(np.median(np.abs(z[acc] / truth[acc] - 1.0)))
