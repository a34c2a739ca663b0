"""What mbavo_pairs_filter_depths costs beside the refinement it shares its evaluation with and beside the route a caller had before
it, at 640 x 480 with 4 pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects.  Inside one process,
interleaved, `reps` repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max:
  filter     mbavo_pairs_filter_depths(level = -1, apply = 1) with records
  refine     mbavo_pairs_refine_depths(level = -1, apply = 1) with records
  composed   the caller's own filter: mbavo_pairs_refine_depths(level = -1, apply = 0) with d_g, d_h into caller arrays, the depths
             gathered from the B x L keypoint arrays, the same fusion as torch elementwise ops on B x sum(cap) tensors (state in
             caller tensors), and the fused depths scattered back through the B x L d_kp_z pointers
The depths are put back to their start before every repetition (not timed); the filter's state and the caller's are NOT, so later
repetitions run with grown information and more gating, which changes no route's work per keypoint.  On grid objects the composed
route is dominated by its 2 x B x L small copies issued from Python (a gather and a scatter per (pair, level)), not by the fusion;
a caller who knows the arena's layout could do either in one indexed copy, so the every-candidate figure is the fairer one to
quote.  Records, not gates: the expectation to confirm or refute is filter within a few percent of refine and clearly under composed.
Usage: python tools/pairs_filter_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r31_pairs_filter.txt): what the file holds above the line
   "# ---- times" is kept, the times and one JSON line per B follow it"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_undistort_bench import H, L_LEVELS, THRESH, W, inputs, mmm, timed

MARK = "# ---- times"
ROUTES = ("filter", "refine", "composed")
OPTS = dict(prior_rel_sigma=0.1, sigma_i=2.0, gate_chi2=9.0)


def device_view(ptr, n, device):
    """n doubles at a raw device pointer as a torch tensor (no copy)."""
    import torch
    iface = {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(type("_DeviceSpan", (), {"__cuda_array_interface__": iface})(), device=device)


def torch_fusion(D, g, h, mu, info, n_obs, n_rej, valid, P, min_info=0.0, max_rel_step=0.25, z_min=1e-2, sigma_i=2.0, gate_chi2=9.0):
    """include/mbavo.h, mbavo_pairs_filter_depths step 4, as elementwise torch ops; returns the fused depths."""
    import torch
    s2 = sigma_i * sigma_i
    rho_c, DD = 1.0 / D, D * D
    g_rho, h_rho = -(DD * g), (DD * DD) * h
    hm = h_rho / s2
    cand = (valid == P) & (hm > min_info) & (h_rho > 0.0)
    e = (rho_c - g_rho / h_rho) - mu
    c2 = (e * e) * ((info * hm) / (info + hm))
    rejected = cand & (info > 0.0) & (c2 > gate_chi2)
    A = info + hm
    m = max_rel_step * rho_c
    d_rho = torch.minimum(torch.maximum((info * (mu - rho_c) - g_rho / s2) / A, -m), m)
    rho_n = rho_c + d_rho
    D_new = 1.0 / rho_n
    fused = cand & ~rejected & torch.isfinite(D_new) & (D_new >= z_min)
    mu.copy_(torch.where(fused, rho_n, mu))
    info.copy_(torch.where(fused, A, info))
    n_obs.add_(fused.to(torch.int32))
    n_rej.add_(rejected.to(torch.int32))
    return torch.where(fused, D_new, D)


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, k = %d, S = 8, P = 8, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, k, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        caps = pb.capacities()
        off = np.concatenate([[0], np.cumsum(caps)])
        n = int(off[-1])
        P = int(pb.array[0].P)
        views = [device_view(pb.array[e].d_kp_z, int(pb.array[e].K), dev) if pb.array[e].K else None for e in range(B * L_LEVELS)]
        where = [(e // L_LEVELS, int(off[e % L_LEVELS])) for e in range(B * L_LEVELS)]
        start = [None if v is None else v.clone() for v in views]
        mk = lambda dt, fill=0: torch.full((B, n), fill, dtype=dt, device=dev)
        g, h, valid, D = mk(torch.float64), mk(torch.float64), mk(torch.int32), mk(torch.float64, 1.0)
        mu, info, n_obs, n_rej = mk(torch.float64), mk(torch.float64), mk(torch.int32), mk(torch.int32)

        def gather():
            for v, (b, o) in zip(views, where):
                if v is not None:
                    D[b, o:o + v.numel()].copy_(v)

        def restore():
            for v, s in zip(views, start):
                if v is not None:
                    v.copy_(s)

        def composed():
            rc, _ = pb.refine_depths(level=-1, apply=False, g=g, h=h, valid=valid)
            assert rc == 0, rc
            gather()
            D_new = torch_fusion(D, g, h, mu, info, n_obs, n_rej, valid, P)
            for v, (b, o) in zip(views, where):
                if v is not None:
                    v.copy_(D_new[b, o:o + v.numel()])

        def filt():
            rc, _ = pb.filter_depths(level=-1, apply=True, **OPTS)
            assert rc == 0, rc

        def refine():
            rc, _ = pb.refine_depths(level=-1, apply=True)
            assert rc == 0, rc

        # the caller's state seeded as the filter seeds its own (not timed)
        gather()
        mu.copy_(1.0 / D)
        info.copy_(1.0 / ((OPTS["prior_rel_sigma"] * mu) * (OPTS["prior_rel_sigma"] * mu)))
        calls = {"filter": filt, "refine": refine, "composed": composed}
        t = {key: [] for key in ROUTES}
        for rep in range(reps + 2):
            for key in ROUTES:
                restore()
                v = timed(calls[key])
                if rep >= 2:
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        name = "every candidate" if dense else "grid"
        r = {key: mmm(v) for key, v in t.items()}
        r.update(filter_over_refine=round(med["filter"] / med["refine"], 4), composed_over_filter=round(med["composed"] / med["filter"], 3),
                 K0_mean=float(counts[:, 0].mean()), stats=pb.filter_stats())
        out["routes"][name] = r
        emit("  %-15s K0 %.0f: filter %s  refine %s  composed %s; filter / refine %.3f, composed / filter %.2f; filter stats %s"
             % (name, r["K0_mean"], r["filter"], r["refine"], r["composed"], r["filter_over_refine"], r["composed_over_filter"], r["stats"]))
        pb.close()
        del views, start, g, h, valid, D, mu, info, n_obs, n_rej
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r31_pairs_filter.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    head = open(out_path).read().split(MARK)[0] if os.path.exists(out_path) else ""
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(ctx, B, emit) for B in Bs]
    for r in results:
        emit(json.dumps(r))
    with open(out_path, "w") as f:
        f.write(head + MARK + " (python tools/pairs_filter_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
