"""What mbavo_pairs_carry_save + mbavo_pairs_carry_adopt cost beside the route a caller had before them and beside one smoothing, at
640 x 480 with 4 pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects (radius 2, deflate 0.8, min_support 1,
max_rel_diff 0.1, apply 1, every pair listed, one small rigid motion for all).  Inside one process, interleaved, `reps` repetitions
each after a warm-up, every repetition between two device synchronisations; min / median / max:
  save       mbavo_pairs_carry_save with records: warp and index, two launches
  adopt      mbavo_pairs_carry_adopt(apply = 1) with records on the keypoints as they are: one launch
  transfer   the composed route's first step: every keypoint coordinate and depth of the object gathered on the device and read back,
             and the filter's mu and info read back whole
  host       the composed route's middle: the warp of the save in numpy, vectorised, on PAIR 0 ALONE, into a level-0 point list; the
             pairs are independent, so a caller's B pairs cost B times this, which the line reports as `host x B` -- an
             extrapolation, and of numpy, not of compiled code
  points     the composed route's last step: mbavo_pairs_update_points for every pair, fed with that point list (pair 0's, B times);
             the list is cut to the smallest level's capacity, the longest the call takes; it holds the upload of the points AND the
             keyframe update itself, which the device route needs too (its update is not in `save + adopt`), so composed
             is given with and without it
  smooth     ONE mbavo_pairs_smooth_depths(radius 2, level = -1, apply = 0) with records on a standing index, for scale
The object is prepared again from the same inputs before every repetition (not timed).  Records, not gates.
Usage: python tools/pairs_carry_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r34_pairs_carry.txt): what the file holds above the line
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
ROUTES = ("save", "adopt", "transfer", "host", "smooth", "points")  # (points last: it rewrites the keypoints)
RADIUS, DEFLATE = 2, 0.8
ADOPT = dict(min_support=1, max_rel_diff=0.1)
_Q = np.array([0.004, -0.006, 0.003, 1.0])
POSE = np.concatenate([[0.02, -0.01, 0.03], _Q / np.linalg.norm(_Q)])


def host_warp(levels, intr, T):
    """The save's warp of one pair on the host: levels = [(H, W, xy K x 2, z K)]; returns the level-0 point list (xy, z) a caller
    would hand to update_points (the carried points of level 0, at their rounded pixels)."""
    x, y, z, w = T[3:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    out = None
    for l, (h, wd, xy, d) in enumerate(levels):
        fx, fy, cx, cy = (v / (1 << l) for v in intr)
        ray = np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(d))], 1)
        Xn = (ray * d[:, None] - T[:3]) @ R
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = np.floor(fx * Xn[:, 0] / Xn[:, 2] + cx + 0.5), np.floor(fy * Xn[:, 1] / Xn[:, 2] + cy + 0.5)
        ok = np.isfinite(d) & (d > 0) & (Xn[:, 2] >= 1e-2) & (u >= 0) & (u < wd) & (v >= 0) & (v < h)
        if l == 0:
            out = (np.stack([u[ok], v[ok]], 1), Xn[ok, 2])
    return out


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    listed, Ts = list(range(B)), np.tile(POSE, (B, 1))
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "radius": RADIUS, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        assert pb.filter_depths(level=-1, prior_rel_sigma=0.1)[0] == 0
        st = pb.filter_state()
        # every keypoint depth / coordinate pair of the object as one index into the span of the arena that holds them
        ents = [(int(pb.array[e].d_kp_z), int(pb.array[e].d_kp_xy), int(pb.array[e].K)) for e in range(B * L_LEVELS) if pb.array[e].K]
        base = min(min(p, q) for p, q, _ in ents)
        span_n = max(max((p - base) // 8 + K, (q - base) // 8 + 2 * K) for p, q, K in ents)
        assert span_n <= pb.stats()[3] // 8, "the keypoints lie in the object's one arena"
        span = device_view(base, span_n, dev)
        idx = torch.cat([torch.arange(K, device=dev, dtype=torch.int64) + (p - base) // 8 for p, _, K in ents]
                        + [torch.arange(2 * K, device=dev, dtype=torch.int64) + (q - base) // 8 for _, q, K in ents])
        lv = []
        for l in range(L_LEVELS):
            q = pb.array[l]
            lv.append((int(q.H), int(q.W), device_view(int(q.d_kp_xy), 2 * q.K, dev).cpu().numpy().reshape(-1, 2).copy(),
                       device_view(int(q.d_kp_z), q.K, dev).cpu().numpy().copy()))
        n_max = min(pb.capacities())  # (a point list may not be longer than the smallest level's capacity)
        pts = [tuple(v[:n_max] for v in host_warp(lv, pb.intr, POSE))] * B
        name = "every candidate" if dense else "grid"
        out["routes"][name] = {"K0_mean": float(counts[:, 0].mean()), "K_per_pair_mean": float(counts.sum(1).mean()), "points_per_pair": len(pts[0][1])}

        def save():
            rc, _ = pb.carry_save(listed, Ts, RADIUS, deflate=DEFLATE)
            assert rc == 0, rc

        def adopt():
            rc, _ = pb.carry_adopt(listed, apply=True, **ADOPT)
            assert rc == 0, rc

        def transfer():
            span[idx].cpu()
            st["mu"].cpu()
            st["info"].cpu()

        def points():
            pb.update_points(None, listed, sharp, pts)

        def smooth():
            rc, _ = pb.smooth_depths(RADIUS, level=-1, apply=False, min_support=2, max_rel_diff=0.25, fill=True)
            assert rc == 0, rc

        t = {key: [] for key in ROUTES}
        for rep in range(reps + 2):
            pb.prepare(sharp, z, blur)
            smooth()  # (the index of the smoothing stands from here on)
            for key in ROUTES:
                if key == "host":
                    t0 = time.perf_counter()
                    host_warp(lv, pb.intr, POSE)
                    v = 1e3 * (time.perf_counter() - t0)
                else:
                    v = timed({"save": save, "adopt": adopt, "transfer": transfer, "points": points, "smooth": smooth}[key])
                if key == "save":
                    assert pb.carry_stats()[0][0] == 2
                if key == "adopt":
                    assert pb.carry_stats()[1][0] == 1
                if rep >= 2:
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        res = {key: mmm(v) for key, v in t.items()}
        device = med["save"] + med["adopt"]
        composed = med["transfer"] + B * med["host"]
        res.update(save_plus_adopt=round(device, 3), host_x_B=round(B * med["host"], 3), composed_without_update=round(composed, 3),
                   composed=round(composed + med["points"], 3), composed_without_update_over_device=round(composed / device, 2),
                   transfer_over_device=round(med["transfer"] / device, 2), device_over_smooth=round(device / med["smooth"], 2))
        out["routes"][name].update(res)
        emit("  %-15s K/pair %.0f: save %s  adopt %s  transfer %s  host (pair 0) %s, host x B %.1f  points %s  smooth %s; save + adopt %.3f, "
             "transfer / (save + adopt) %.2f, composed without the update / (save + adopt) %.1f, (save + adopt) / smooth %.2f"
             % (name, out["routes"][name]["K_per_pair_mean"], res["save"], res["adopt"], res["transfer"], res["host"], res["host_x_B"], res["points"],
                res["smooth"], device, res["transfer_over_device"], res["composed_without_update_over_device"], res["device_over_smooth"]))
        pb.close()
        del span, idx, st
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r34_pairs_carry.txt")
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
        f.write(head + MARK + " (python tools/pairs_carry_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
