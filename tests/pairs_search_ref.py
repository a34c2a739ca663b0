"""numpy restatement of mbavo_pairs_search_depths (include/mbavo.h, steps 1 - 8) on one rebuilt entry (helper, no test in it): the
candidates, the cost volume on top of pairs_refine_ref.keypoints(e, poses, z=...), the selection as a pure function of a volume,
the acceptance and the record sums in the order of pairs_refine_ref.lane_sum.  float64, operation by operation as the header
writes them."""
import ctypes as C

import numpy as np

import pairs_refine_ref as ref

E_RANGE = ref.E_RANGE


def candidates(z, ND, rho_lo, rho_hi, relative=0):
    """Step 1 for keypoints at depths z: (lo K, step K, rho K x ND, D K x ND)."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo = rho_lo / z if relative else np.full(z.size, float(rho_lo))
        hi = rho_hi / z if relative else np.full(z.size, float(rho_hi))
        step = (hi - lo) / float(ND - 1)
        rho = lo[:, None] + np.arange(ND, dtype=np.float64)[None, :] * step[:, None]
        return lo, step, rho, 1.0 / rho


def volume(e, pose_list, D):
    """Step 2: K x ND costs at the candidate depths D (K x ND), NaN where a candidate is not full."""
    vol = np.full(D.shape, np.nan)
    for d in range(D.shape[1]):
        r = ref.keypoints(e, pose_list, z=D[:, d])
        vol[:, d] = np.where(r["full"], r["cost"], np.nan)
    return vol


def select(vol, lo, step):
    """Steps 3 and 4 on a K x ND volume (NaN: not full): dict(best, num_full (int32), cost_best, cost_second, rho, curv (float64),
    parabola (bool)).  Comparisons only up to the parabola."""
    vol = np.asarray(vol, np.float64)
    K, ND = vol.shape
    lo, step = np.broadcast_to(np.asarray(lo, np.float64), (K,)), np.broadcast_to(np.asarray(step, np.float64), (K,))
    out = dict(best=np.full(K, -1, np.int32), num_full=np.zeros(K, np.int32), cost_best=np.full(K, np.nan), cost_second=np.full(K, np.nan),
               rho=np.full(K, np.nan), curv=np.zeros(K), parabola=np.zeros(K, bool))
    for i in range(K):
        c = vol[i]
        full = ~np.isnan(c)
        out["num_full"][i] = full.sum()
        best = -1
        for d in range(ND):
            if full[d] and (best < 0 or c[d] < c[best]):
                best = d
        if best < 0:
            continue
        second = np.nan
        for d in range(ND):
            if full[d] and abs(d - best) > 1 and (np.isnan(second) or c[d] < second):
                second = c[d]
        rho, curv = lo[i] + float(best) * step[i], 0.0
        if 0 < best < ND - 1 and full[best - 1] and full[best + 1]:
            with np.errstate(over="ignore"):
                den = (c[best - 1] - 2.0 * c[best]) + c[best + 1]
            if den > 0.0:
                delta = 0.5 * (c[best - 1] - c[best + 1]) / den
                delta = min(max(delta, -0.5), 0.5)
                rho = rho + delta * step[i]
                curv = den / (step[i] * step[i])
                out["parabola"][i] = True
        out["best"][i], out["cost_best"][i], out["cost_second"][i], out["rho"][i], out["curv"][i] = best, c[best], second, rho, curv
    return out


def accept(sel, min_ratio=0.0, min_curv=0.0, z_min=0.0, z_max=0.0):
    """Step 5: (accepted K bool, z_new K (NaN where not accepted), ratio K (cost_best / cost_second, 0 where there is none))."""
    z_min = 1e-2 if z_min == 0 else z_min
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ok = sel["best"] >= 0
        if min_ratio != 0:
            ok &= sel["cost_second"] >= min_ratio * sel["cost_best"]  # (False for a NaN runner-up)
        ok &= np.where(sel["parabola"], sel["curv"] > min_curv, min_curv == 0)
        z_new = 1.0 / sel["rho"]
        ok &= np.isfinite(z_new) & (z_new >= z_min) & ((z_max == 0) | (z_new <= z_max))
        has = ~np.isnan(sel["cost_second"]) & (sel["cost_second"] != 0)
        ratio = np.where(has, sel["cost_best"] / np.where(has, sel["cost_second"], 1.0), 0.0)
    return ok, np.where(ok, z_new, np.nan), ratio


def records(sel, accepted, ratio, P, cap):
    """Step 8 from a selection: dict(num_searched, num_accepted, cost, sum_ratio)."""
    return dict(num_searched=int((sel["best"] >= 0).sum()), num_accepted=int(accepted.sum()),
                cost=ref.lane_sum(np.where(accepted, sel["cost_best"], 0.0), P, cap), sum_ratio=ref.lane_sum(np.where(accepted, ratio, 0.0), P, cap))


def search(lib, capi, e, k, cap, ND, rho_lo, rho_hi, relative=0, **opts):
    """The whole call on one entry whose level has keypoint capacity `cap`."""
    if not ref.on_knots(e, k):
        return dict(status=E_RANGE, num_keypoints=e["K"], num_searched=0, num_accepted=0, cost=float("nan"), sum_ratio=float("nan"))
    lo, step, rho, D = candidates(e["z"], ND, rho_lo, rho_hi, relative)
    vol = volume(e, ref.poses(lib, capi, e, k), D)
    sel = select(vol, lo, step)
    accepted, z_new, ratio = accept(sel, **opts)
    out = dict(sel, status=0, num_keypoints=e["K"], volume=vol, accepted=accepted, z_new=np.where(accepted, z_new, e["z"]), step=step, D=D)
    out.update(records(sel, accepted, ratio, e["P"], cap))
    return out


def opts_struct(capi, num_candidates=8, rho_lo=0.25, rho_hi=1.0, level=-1, apply=0, relative=0, min_ratio=0.0, min_curv=0.0, z_min=0.0, z_max=0.0):
    o = capi.PairsSearchOpts()
    o.level, o.apply, o.num_candidates, o.relative = level, apply, num_candidates, relative
    o.rho_lo, o.rho_hi, o.min_ratio, o.min_curv, o.z_min, o.z_max = rho_lo, rho_hi, min_ratio, min_curv, z_min, z_max
    return o


def call(lib, handle, o, out=None, rho=None, cost_best=None, cost_second=None, curv=None, best=None, num_full=None, volume=None):
    """The raw entry point with optional ctypes records and device pointers (ints)."""
    return lib.mbavo_pairs_search_depths(handle, None if o is None else C.byref(o), out, rho, cost_best, cost_second, curv, best, num_full, volume)
