"""What mbavo_pairs_search_depths costs beside the route a caller had before it and beside one refinement, at 640 x 480 with 4
pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects, at ND = 8, 16, 32, 64 candidates on the absolute
range [0.3, 2.2] (the depth maps hold z in [0.5, 3]).  Inside one process, interleaved, `reps` repetitions each after a warm-up,
every repetition between two device synchronisations; min / median / max:
  search     mbavo_pairs_search_depths(level = -1, apply = 0) with records, d_best and d_rho into caller arrays
  composed   the caller's own search: ND x (candidate d's depth written into every keypoint depth of the object +
             mbavo_pairs_refine_depths(level = -1, apply = 0) with d_cost, d_valid into caller arrays, no records, nothing waited
             for + a streaming argmin over the full candidates as torch elementwise ops on B x sum(cap) tensors)
  refine     ONE mbavo_pairs_refine_depths(level = -1, apply = 0) with records
The composed route writes its depths in ONE indexed fill over the span of the arena that holds every (pair, level)'s depths (the
index is built once, not timed), so what it pays per candidate is one fill, one refinement launch with its copy of the options
and four elementwise kernels -- not B x L small copies issued from Python.  It has no parabola, curvature or runner-up.  The
depths are put back to their start after every composed repetition (not timed).  Records, not gates: the expectation to confirm
or refute is search clearly under ND x refine and under composed.
Usage: python tools/pairs_search_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r32_pairs_search.txt): what the file holds above the line
   "# ---- times" is kept, the times and one JSON line per B follow it"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_filter_bench import device_view
from pairs_undistort_bench import H, L_LEVELS, THRESH, W, inputs, mmm, timed

MARK = "# ---- times"
ROUTES = ("search", "composed", "refine")
NDS = (8, 16, 32, 64)
RHO_LO, RHO_HI = 0.3, 2.2


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "rho": [RHO_LO, RHO_HI], "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, k = %d, S = 8, P = 8, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, k, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        n = int(sum(pb.capacities()))
        P = int(pb.array[0].P)
        # every keypoint depth of the object as one index into the span of the arena between the lowest and the highest of them
        ents = [(int(pb.array[e].d_kp_z), int(pb.array[e].K)) for e in range(B * L_LEVELS) if pb.array[e].K]
        base = min(p for p, _ in ents)
        span_n = max((p - base) // 8 + K for p, K in ents)
        assert all((p - base) % 8 == 0 for p, _ in ents) and span_n <= pb.stats()[3] // 8, "the depths lie in the object's one arena"
        span = device_view(base, span_n, dev)
        idx = torch.cat([torch.arange(K, device=dev, dtype=torch.int64) + (p - base) // 8 for p, K in ents])
        assert int(idx.min()) >= 0 and int(idx.max()) < span_n
        start = span[idx].clone()
        mk = lambda dt, fill=0: torch.full((B, n), fill, dtype=dt, device=dev)
        cost, valid = mk(torch.float64), mk(torch.int32)
        c_best, i_best = mk(torch.float64), mk(torch.int32)
        s_best, s_rho = mk(torch.int32), mk(torch.float64)
        name = "every candidate" if dense else "grid"
        out["routes"][name] = {"K0_mean": float(counts[:, 0].mean())}

        def refine():
            rc, _ = pb.refine_depths(level=-1, apply=False)
            assert rc == 0, rc

        for ND in NDS:
            step = (RHO_HI - RHO_LO) / (ND - 1)

            def search():
                rc, _ = pb.search_depths(ND, RHO_LO, RHO_HI, level=-1, apply=False, best=s_best, rho=s_rho)
                assert rc == 0, rc

            def composed():
                c_best.fill_(float("inf"))
                i_best.fill_(-1)
                for d in range(ND):
                    span.index_fill_(0, idx, 1.0 / (RHO_LO + d * step))
                    rc, _ = pb.refine_depths(level=-1, apply=False, cost=cost, valid=valid, want_records=False)
                    assert rc == 0, rc
                    better = (valid == P) & (cost < c_best)
                    c_best.copy_(torch.where(better, cost, c_best))
                    i_best.masked_fill_(better, d)

            calls = {"search": search, "composed": composed, "refine": refine}
            t = {key: [] for key in ROUTES}
            for rep in range(reps + 2):
                for key in ROUTES:
                    v = timed(calls[key])
                    if key == "composed":
                        span.index_copy_(0, idx, start)
                    if rep >= 2:
                        t[key].append(v)
            med = {key: statistics.median(v) for key, v in t.items()}
            r = {key: mmm(v) for key, v in t.items()}
            r.update(search_over_refine=round(med["search"] / med["refine"], 3), composed_over_search=round(med["composed"] / med["search"], 3),
                     stats=pb.search_stats())
            out["routes"][name]["ND %d" % ND] = r
            emit("  %-15s K0 %.0f ND %2d: search %s  composed %s  refine %s; search / refine %.2f (ND x refine: %d), composed / search %.2f"
                 % (name, out["routes"][name]["K0_mean"], ND, r["search"], r["composed"], r["refine"], r["search_over_refine"], ND, r["composed_over_search"]))
        pb.close()
        del span, idx, start, cost, valid, c_best, i_best, s_best, s_rho
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r32_pairs_search.txt")
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
        f.write(head + MARK + " (python tools/pairs_search_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
