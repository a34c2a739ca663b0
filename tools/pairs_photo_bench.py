"""What mbavo_pairs_match_brightness costs beside one depth refinement and beside the route a caller had before it, at 640 x 480
with 4 pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects.  Inside one process, interleaved, `reps`
repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max:
  fit R l    mbavo_pairs_match_brightness(rounds = R, level = l, apply = 0) with records, for R = 1 and 3 at level L - 1 and 0
  apply R l  the same call with apply = 1 (the level-0 map and the pyramid launches on top)
  refine     ONE mbavo_pairs_refine_depths(level = 0, apply = 0) with records, for scale
  the caller-composed route the call replaces, as a caller must write it today:
  transfer   the level-0 keyframes and current frames of all pairs read back
  host       numpy: a least-squares gain and offset per pair from the whole frames (no alignment, no Huber weight: what a caller
             can do without the evaluation), the corrected frames
  update     mbavo_pairs_update with the corrected frames (n_key = 0)
The blurred frames are restored by an update before every repetition (not timed).  Records, not gates.
Usage: python tools/pairs_photo_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r42_pairs_photo.txt): what the file holds above the line
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


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    k, N = 2, 2
    dev = "cuda:%d" % ctx.device_id
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d in ms, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        pb = workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=k, N=N, cell=30, thresh=THRESH, every_candidate=dense)
        counts = pb.prepare(sharp, z, blur)
        assert pb.set_states(pb.initial_states(0.0, 0.1)) == 0 and pb.predict(np.full(B, 0.05), np.full(B, 0.02)) == 0
        name = "every candidate" if dense else "grid"
        out["routes"][name] = {"K0_mean": float(counts[:, 0].mean()), "K_top_mean": float(counts[:, L_LEVELS - 1].mean())}
        host = {}

        def fit(R, level, apply):
            def run():
                rc, rec = pb.match_brightness(level=level, rounds=R, apply=apply)
                assert rc == 0, rc
                host["ok"] = sum(r.status == 0 for r in rec)
            return run

        def refine():
            rc, _ = pb.refine_depths(level=0, apply=False)
            assert rc == 0, rc

        def transfer():
            host["sharp"], host["blur"] = sharp.cpu().numpy().reshape(B, -1), blur.cpu().numpy().reshape(B, -1)

        def compose():
            s, c = host["sharp"].astype(np.float64), host["blur"].astype(np.float64)
            n = s.shape[1]
            sx, sy = s.sum(1), c.sum(1)
            det = n * (s * s).sum(1) - sx * sx
            a = (n * (s * c).sum(1) - sx * sy) / det
            b = (sy - a * sx) / n
            host["fixed"] = np.clip(np.rint((c - b[:, None]) / a[:, None]), 0, 255).astype(np.uint8).reshape(B, H, W)

        def update():
            pb.update(torch.from_numpy(host["fixed"]).to(dev))

        calls = {"refine": refine, "transfer": transfer, "host": compose, "update": update}
        for R in (1, 3):
            for level in (L_LEVELS - 1, 0):
                calls["fit %d l%d" % (R, level)] = fit(R, level, False)
                calls["apply %d l%d" % (R, level)] = fit(R, level, True)
        order = [key for key in calls if key.startswith("fit")] + ["refine", "transfer", "host", "update"] + [key for key in calls if key.startswith("apply")]
        t = {key: [] for key in order}
        for rep in range(reps + 2):
            for key in order:
                if key.startswith("apply") or key == "update":
                    pb.update(blur)  # (the frames as they came)
                v = timed(calls[key])
                if rep >= 2:
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        res = {key: mmm(v) for key, v in t.items()}
        composed = med["transfer"] + med["host"] + med["update"]
        res.update(pairs_fitted=int(host["ok"]), composed=round(composed, 3), composed_over_apply=round(composed / med["apply 3 l%d" % (L_LEVELS - 1)], 1),
                   fit_over_refine=round(med["fit 3 l0"] / med["refine"], 3))
        out["routes"][name].update(res)
        emit("  %-15s K0 %.0f, K top %.0f: %s | refine %s | composed: transfer %s  host %s  update %s = %.3f, %.1f x apply 3 l%d; fit 3 l0 / refine %.3f"
             % (name, out["routes"][name]["K0_mean"], out["routes"][name]["K_top_mean"], "  ".join("%s %s" % (key, res[key]) for key in order if key[0] in "fa"),
                res["refine"], res["transfer"], res["host"], res["update"], composed, res["composed_over_apply"], L_LEVELS - 1, res["fit_over_refine"]))
        pb.close()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r42_pairs_photo.txt")
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
        f.write(head + MARK + " (python tools/pairs_photo_bench.py %s, one MI355X)\n" % " ".join(str(b) for b in Bs) + "\n".join(text) + "\n")
    ctx.close()
