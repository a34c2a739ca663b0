"""numpy restatement of mbavo_pairs_filter_depths (include/mbavo.h, steps 1 - 6) on one rebuilt entry (helper, no test in it):
seeding and fusion on top of pairs_refine_ref's g / h / valid / cost, float64, operation by operation as the header writes them.

A state is dict(mu, info (float64 K), n_obs, n_rej (int32 K)).  `filter` takes an entry (pairs_oracle.read_entry), the state before
the call and the seed flag, and returns the state after, z_new, the fused and rejected masks and the record sums in the order of
pairs_refine_ref.lane_sum."""
import ctypes as C

import numpy as np

import pairs_refine_ref as ref

E_RANGE = ref.E_RANGE
OPTS = ("min_info", "max_rel_step", "z_min", "z_max", "sigma_i", "prior_rel_sigma", "gate_chi2")


def seed(z, prior_rel_sigma=0.0):
    """Step 3: the state a (pair, level) starts with at depths z."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = 1.0 / z
        info = np.zeros(z.size) if prior_rel_sigma == 0 else 1.0 / ((prior_rel_sigma * mu) * (prior_rel_sigma * mu))
    return dict(mu=mu, info=info, n_obs=np.zeros(z.size, np.int32), n_rej=np.zeros(z.size, np.int32))


def empty_state(K):
    return dict(mu=np.zeros(K), info=np.zeros(K), n_obs=np.zeros(K, np.int32), n_rej=np.zeros(K, np.int32))


def fuse(z, g, h, full, state, min_info=0.0, max_rel_step=0.0, z_min=0.0, z_max=0.0, sigma_i=0.0, prior_rel_sigma=0.0, gate_chi2=0.0):
    """Step 4 on K keypoints: dict(state (after), z_new (z where not fused), cand, fused, rejected (K bool), c2 (K; nan where the
    gate does not apply), A, rel (K; 0 where not fused), h_rho)."""
    max_rel_step = 0.25 if max_rel_step == 0 else max_rel_step
    z_min = 1e-2 if z_min == 0 else z_min
    sigma_i = 1.0 if sigma_i == 0 else sigma_i
    z = np.asarray(z, np.float64)
    mu, info = state["mu"], state["info"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s2 = sigma_i * sigma_i
        rho_c, DD = 1.0 / z, z * z
        g_rho, h_rho = -(DD * g), (DD * DD) * h
        hm = h_rho / s2
        cand = full & (hm > min_info) & (h_rho > 0.0)
        gated = cand & (info > 0.0) if gate_chi2 > 0 else np.zeros(z.size, bool)
        rho_m = rho_c - g_rho / h_rho
        e = rho_m - mu
        c2 = np.where(gated, (e * e) * ((info * hm) / (info + hm)), np.nan)
        rejected = gated & (c2 > gate_chi2)
        A = info + hm
        bv = info * (mu - rho_c) - g_rho / s2
        m = max_rel_step * rho_c
        d_rho = bv / A
        d_rho = np.where(d_rho > m, m, d_rho)
        d_rho = np.where(d_rho < -m, -m, d_rho)
        rho_n = rho_c + d_rho
        z_new = 1.0 / rho_n
        fused = cand & ~rejected & np.isfinite(z_new) & (z_new >= z_min) & ((z_max == 0) | (z_new <= z_max))
        rel = np.where(fused, d_rho / rho_c, 0.0)
    after = dict(mu=np.where(fused, rho_n, mu), info=np.where(fused, A, info), n_obs=(state["n_obs"] + fused).astype(np.int32),
                 n_rej=(state["n_rej"] + rejected).astype(np.int32))
    return dict(state=after, z_new=np.where(fused, z_new, z), cand=cand, fused=fused, rejected=rejected, c2=c2, A=np.where(fused, A, 0.0), rel=rel,
                h_rho=h_rho)


def filter(lib, capi, e, k, cap, state, seeded, g_scale=1.0, **opts):
    """The whole call on one entry whose level has keypoint capacity `cap`.  g_scale multiplies g before the fusion (the CPU
    check of the gate's margin)."""
    opts = {key: v for key, v in opts.items() if key != "reset"}  # (what reset asks for is in `seeded`)
    prior = opts.get("prior_rel_sigma", 0.0)
    before = seed(e["z"], prior) if seeded else state
    if not ref.on_knots(e, k):
        nan = float("nan")
        return dict(status=E_RANGE, num_keypoints=e["K"], num_full=0, num_fused=0, num_rejected=0, seeded=int(seeded), cost=nan, sum_info=nan,
                    sum_sq_rel=nan, state=before, z_new=e["z"].copy(), fused=np.zeros(e["K"], bool), rejected=np.zeros(e["K"], bool))
    r = ref.keypoints(e, ref.poses(lib, capi, e, k))
    f = fuse(e["z"], r["g"] * g_scale, r["h"], r["full"], before, **opts)
    P = e["P"]
    r.update(f)
    r.update(status=0, num_keypoints=e["K"], num_full=int(r["full"].sum()), num_fused=int(f["fused"].sum()), num_rejected=int(f["rejected"].sum()),
             seeded=int(seeded), sum_cost=ref.lane_sum(np.where(r["full"], r["cost"], 0.0), P, cap), sum_info=ref.lane_sum(f["A"], P, cap),
             sum_sq_rel=ref.lane_sum(f["rel"] * f["rel"], P, cap))
    return r


def opts_struct(capi, level=-1, apply=0, reset=0, **kw):
    o = capi.PairsFilterOpts()
    o.level, o.apply, o.reset = level, apply, reset
    for key, v in kw.items():
        assert key in OPTS, key
        setattr(o, key, v)
    return o


def call(lib, handle, o, out=None):
    """The raw entry point with optional ctypes records."""
    return lib.mbavo_pairs_filter_depths(handle, None if o is None else C.byref(o), out)
