"""What mbavo_pairs_prune_keypoints costs beside the route a caller had before it and beside one smoothing and one filter call, at
640 x 480 with 4 pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects, one keypoint in four dropped at
random by a flag byte (the same bytes for every route).  Inside one process, interleaved, `reps` repetitions each after a warm-up,
every repetition between two device synchronisations; min / median / max:
  prune      mbavo_pairs_prune_keypoints(level = -1, apply = 1) with records, every pair: one launch, one read-back
  count      the same call with apply = 0 and records
  smooth     ONE mbavo_pairs_smooth_depths(radius 2, level = -1, apply = 0) with records on a standing index, for scale
  filter     ONE mbavo_pairs_filter_depths(level = -1, apply = 0) with records, for scale
  the caller-composed route the call replaces, as a caller must write it today, step by step:
  transfer   every keypoint coordinate and depth of the object gathered on the device and read back, the flag bytes and the
             filter's four state arrays read back whole
  host       numpy: every (pair, level)'s state compacted by the flags into a host copy, level 0's keypoints compacted into one
             point list per pair (cut to the smallest level's capacity, the longest list update_points takes)
  points     mbavo_pairs_update_points for all pairs with those lists -- it makes every level's keypoints from the level-0 list
             (so each level is NOT pruned on its own flags), rewrites the keyframe images and gradients, marks every filter state
             for seeding and every spatial index for rebuilding: what the prune call preserves
  writeback  the four compacted state arrays copied back to the device
The object is prepared and filtered again from the same inputs before every repetition (not timed).  Records, not gates.
Usage: python tools/pairs_prune_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r36_pairs_prune.txt): what the file holds above the line
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
ROUTES = ("count", "smooth", "filter", "transfer", "host", "prune", "points", "writeback")  # (prune, then points: they change the keypoints)
DROP, STAY = 3, 40


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    listed = list(range(B))
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        assert pb.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0
        st = pb.filter_state()
        cap = pb.capacities()
        off = np.concatenate([[0], np.cumsum(cap)])
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        flags = torch.where(torch.rand((B, sum(cap)), device=dev, generator=gen) < 0.25, DROP, STAY).to(torch.uint8).contiguous()
        ents = [(int(pb.array[e].d_kp_z), int(pb.array[e].d_kp_xy), int(pb.array[e].K)) for e in range(B * L_LEVELS) if pb.array[e].K]
        base = min(min(p, q) for p, q, _ in ents)
        span_n = max(max((p - base) // 8 + K, (q - base) // 8 + 2 * K) for p, q, K in ents)
        span = device_view(base, span_n, dev)
        idx = torch.cat([torch.arange(K, device=dev, dtype=torch.int64) + (p - base) // 8 for p, _, K in ents]
                        + [torch.arange(2 * K, device=dev, dtype=torch.int64) + (q - base) // 8 for _, q, K in ents])
        n_max = min(cap)
        name = "every candidate" if dense else "grid"
        out["routes"][name] = {"K0_mean": float(counts[:, 0].mean()), "K_per_pair_mean": float(counts.sum(1).mean())}
        host = {}

        def prune():
            rc, rec = pb.prune_keypoints(None, level=-1, apply=True, flags=flags, drop_mask=1 << DROP)
            assert rc == 0 and pb.prune_stats()[:2] == (1, 1), rc
            host["kept"] = sum(r.num_kept for r in rec) / max(sum(r.num_before for r in rec), 1)

        def count():
            rc, _ = pb.prune_keypoints(None, level=-1, apply=False, flags=flags, drop_mask=1 << DROP)
            assert rc == 0, rc

        def smooth():
            rc, _ = pb.smooth_depths(2, level=-1, apply=False, min_support=2, max_rel_diff=0.25, fill=True)
            assert rc == 0, rc

        def filt():
            rc, _ = pb.filter_depths(level=-1, apply=False, prior_rel_sigma=0.1)
            assert rc == 0, rc

        def transfer():
            host["kp"] = span[idx].cpu().numpy()
            host["flags"] = flags.cpu().numpy()
            host["state"] = {key: st[key].cpu().numpy() for key in ("mu", "info", "n_obs", "n_rej")}

        def compact():
            kp, fl, state = host["kp"], host["flags"], host["state"]
            nz = sum(K for _, _, K in ents)
            pz, pxy, pts = 0, nz, []
            new = {key: v.copy() for key, v in state.items()}
            for b in range(B):
                for l in range(L_LEVELS):
                    K = int(counts[b, l])
                    if K == 0:
                        continue
                    keep = fl[b, off[l]:off[l] + K] != DROP
                    m = int(keep.sum())
                    for key, v in new.items():
                        v[b, off[l]:off[l] + m] = state[key][b, off[l]:off[l] + K][keep]
                    if l == 0:
                        xy = kp[pxy:pxy + 2 * K].reshape(-1, 2)[keep][:n_max]
                        pts.append((xy, kp[pz:pz + K][keep][:n_max]))
                    pz, pxy = pz + K, pxy + 2 * K
                if counts[b, 0] == 0:
                    pts.append((np.zeros((0, 2)), np.zeros(0)))
            host["pts"], host["new"] = pts, new

        def points():
            pb.update_points(None, listed, sharp, host["pts"])

        def writeback():
            for key, v in host["new"].items():
                st[key].copy_(torch.from_numpy(v))

        calls = {"prune": prune, "count": count, "smooth": smooth, "filter": filt, "transfer": transfer, "host": compact, "points": points,
                 "writeback": writeback}
        t = {key: [] for key in ROUTES}
        for rep in range(reps + 2):
            pb.prepare(sharp, z, blur)
            filt()
            smooth()  # (the index of the smoothing stands from here on)
            for key in ROUTES:
                v = timed(calls[key])
                if rep >= 2:
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        res = {key: mmm(v) for key, v in t.items()}
        composed = med["transfer"] + med["host"] + med["points"] + med["writeback"]
        res.update(kept_share=round(host["kept"], 4), composed=round(composed, 3), composed_over_prune=round(composed / med["prune"], 1),
                   transfer_over_prune=round(med["transfer"] / med["prune"], 1), prune_over_filter=round(med["prune"] / med["filter"], 3),
                   prune_over_smooth=round(med["prune"] / med["smooth"], 3))
        out["routes"][name].update(res)
        emit("  %-15s K/pair %.0f, kept %.3f: prune %s  count %s  smooth %s  filter %s | composed: transfer %s  host %s  points %s  writeback %s; "
             "composed %.3f = %.1f x prune, transfer alone %.1f x prune; prune / filter %.3f, prune / smooth %.3f"
             % (name, out["routes"][name]["K_per_pair_mean"], host["kept"], res["prune"], res["count"], res["smooth"], res["filter"], res["transfer"],
                res["host"], res["points"], res["writeback"], composed, res["composed_over_prune"], res["transfer_over_prune"], res["prune_over_filter"],
                res["prune_over_smooth"]))
        pb.close()
        del span, idx, st, flags
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r36_pairs_prune.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    head = open(out_path).read().split(MARK)[0] if os.path.exists(out_path) else ""
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(ctx, B, emit) for B in Bs]
    for res in results:
        emit(json.dumps(res))
    with open(out_path, "w") as f:
        f.write(head + MARK + " (python tools/pairs_prune_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
