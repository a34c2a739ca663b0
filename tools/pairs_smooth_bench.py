"""What mbavo_pairs_smooth_depths costs beside the route a caller had before it and beside one refinement, at 640 x 480 with 4
pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects, at radius 2, 4 and 8 (min_support 2, max_rel_diff
0.25, fill 1, apply 1; the depth maps hold z in [0.5, 3] per pixel, so most keypoints are filled -- the neighbourhoods are walked
whatever the class).  Inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition between two device
synchronisations; min / median / max:
  first      mbavo_pairs_smooth_depths(level = -1, apply = 1) with records on a stale index: index and gather, two launches (the
             object is prepared again from the same inputs before it, not timed: the same keypoints under a new serial)
  repeat     the same call on the index as it stands: one launch
  transfer   the composed route's two ends alone: every keypoint depth of the object gathered on the device, read back, written
             up again and scattered into the object (one indexed copy each way: the index is built once, not timed)
  host       the composed route's middle: the same sweep in numpy on the host with a grid index (a pixel -> keypoint map per level,
             one vectorised pass per window offset), on PAIR 0 ALONE; the pairs are independent, so a caller's B pairs cost B times
             this, which the line reports as `host x B` -- an extrapolation, and of numpy, not of compiled code
  refine     ONE mbavo_pairs_refine_depths(level = -1, apply = 0) with records, for scale
composed = transfer + host x B.  `transfer` alone is the floor of ANY composed route, however fast its host sweep.  The depths are
put back to their start after every repetition that wrote them (not timed).  Records, not gates.
Usage: python tools/pairs_smooth_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r33_pairs_smooth.txt): what the file holds above the line
   "# ---- times" is kept, the times and one JSON line per B follow it"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_filter_bench import device_view
from pairs_undistort_bench import H, L_LEVELS, THRESH, W, inputs, mmm, timed

MARK = "# ---- times"
ROUTES = ("first", "repeat", "transfer", "host", "refine")
RADII = (2, 4, 8)
OPTS = dict(min_support=2, max_rel_diff=0.25, strength=1.0, fill=True)


def host_sweep(levels, r):
    """One sweep over the levels of one pair on the host: levels = [(H, W, xy K x 2 ints, z K)]; returns the new depths per level."""
    out = []
    for h, w, xy, z in levels:
        K = len(z)
        grid = np.full((h + 2 * r, w + 2 * r), -1, np.int32)  # the index: pixel -> keypoint, a margin of r saves the bounds tests
        x, y = xy[:, 0] + r, xy[:, 1] + r
        grid[y, x] = np.arange(K, dtype=np.int32)
        rho = 1.0 / z
        tol = OPTS["max_rel_diff"] * rho
        swc, src, swn, srn = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros(K)
        nc, nn = np.zeros(K, np.int32), np.zeros(K, np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    continue
                j = grid[y + dy, x + dx]
                has = j >= 0
                rj = np.where(has, rho[np.where(has, j, 0)], 0.0)
                nn += has
                swn += has
                srn += rj
                agree = has & (np.abs(rj - rho) <= tol)
                nc += agree
                swc += agree
                src += np.where(agree, rj, 0.0)
        sup = nc >= OPTS["min_support"]
        fil = ~sup & (nn >= OPTS["min_support"])
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(sup, (rho + OPTS["strength"] * src) / (1.0 + OPTS["strength"] * swc), np.where(fil, srn / swn, rho))
            zn = 1.0 / new
        ok = np.isfinite(zn) & (zn >= 1e-2)
        out.append(np.where(ok, zn, z))
    return out


def bench(ctx, B, emit, reps=7):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "opts": OPTS, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        # every keypoint depth of the object as one index into the span of the arena between the lowest and the highest of them
        ents = [(int(pb.array[e].d_kp_z), int(pb.array[e].K)) for e in range(B * L_LEVELS) if pb.array[e].K]
        base = min(p for p, _ in ents)
        span_n = max((p - base) // 8 + K for p, K in ents)
        assert all((p - base) % 8 == 0 for p, _ in ents) and span_n <= pb.stats()[3] // 8, "the depths lie in the object's one arena"
        span = device_view(base, span_n, dev)
        idx = torch.cat([torch.arange(K, device=dev, dtype=torch.int64) + (p - base) // 8 for p, K in ents])
        start = span[idx].clone()
        # pair 0's levels on the host, for the host sweep
        lv = []
        for l in range(L_LEVELS):
            q = pb.array[l]
            xy = device_view(int(q.d_kp_xy), 2 * q.K, dev).cpu().numpy().reshape(-1, 2).astype(np.int64)
            lv.append((int(q.H), int(q.W), xy, device_view(int(q.d_kp_z), q.K, dev).cpu().numpy().copy()))
        name = "every candidate" if dense else "grid"
        out["routes"][name] = {"K0_mean": float(counts[:, 0].mean()), "K_per_pair_mean": float(counts.sum(1).mean())}

        def refine():
            rc, _ = pb.refine_depths(level=-1, apply=False)
            assert rc == 0, rc

        def transfer():
            host = span[idx].cpu()
            span.index_copy_(0, idx, host.to(dev))

        for r in RADII:
            def smooth():
                rc, _ = pb.smooth_depths(r, level=-1, apply=True, **OPTS)
                assert rc == 0, rc

            t = {key: [] for key in ROUTES}
            launches = {}
            for rep in range(reps + 2):
                for key in ROUTES:
                    if key == "first":  # (the same keypoints written anew: every pair's serial moves, the next call rebuilds every index)
                        pb.prepare(sharp, z, blur)
                    if key == "host":
                        t0 = time.perf_counter()
                        host_sweep(lv, r)
                        v = 1e3 * (time.perf_counter() - t0)
                    else:
                        v = timed({"first": smooth, "repeat": smooth, "transfer": transfer, "refine": refine}[key])
                    if key in ("first", "repeat"):
                        launches[key] = pb.smooth_stats()[0]
                        span.index_copy_(0, idx, start)
                    if rep >= 2:
                        t[key].append(v)
            assert launches == {"first": 2, "repeat": 1}, launches
            med = {key: statistics.median(v) for key, v in t.items()}
            res = {key: mmm(v) for key, v in t.items()}
            composed = med["transfer"] + B * med["host"]
            res.update(host_x_B=round(B * med["host"], 3), composed=round(composed, 3), composed_over_repeat=round(composed / med["repeat"], 2),
                       transfer_over_repeat=round(med["transfer"] / med["repeat"], 2), first_over_repeat=round(med["first"] / med["repeat"], 2),
                       repeat_over_refine=round(med["repeat"] / med["refine"], 2))
            out["routes"][name]["r %d" % r] = res
            emit("  %-15s K/pair %.0f r %d: first %s  repeat %s  transfer %s  host (pair 0) %s, host x B %.1f  refine %s; first / repeat %.2f, "
                 "transfer / repeat %.2f, composed / repeat %.1f, repeat / refine %.2f"
                 % (name, out["routes"][name]["K_per_pair_mean"], r, res["first"], res["repeat"], res["transfer"], res["host"], res["host_x_B"],
                    res["refine"], res["first_over_repeat"], res["transfer_over_repeat"], res["composed_over_repeat"], res["repeat_over_refine"]))
        pb.close()
        del span, idx, start
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r33_pairs_smooth.txt")
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
        f.write(head + MARK + " (python tools/pairs_smooth_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
