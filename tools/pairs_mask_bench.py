"""What caller-supplied masks cost in a batch of keyframe pairs (mbavo_pairs_opts.mask, mbavo_pairs_set_masks), at 640 x 480 with 4
pyramid levels, one camera, grid selection and every candidate.  Inside one process, interleaved, `reps` repetitions each after a
warm-up, every repetition between two device synchronisations; min / median / max and the spread (max - min):
  (a) a mbavo_pairs_prepare with undistort = 1, valid_radius = 2 under a wide `to` camera, against the same with mask = 1 and a
      bonnet mask (a half-ellipse over the lower part of the raw image) set;
  (b) a mbavo_pairs_prepare with undistort = 0, plain, against mask = 1, valid_radius = 2 with the bonnet drawn in the image;
  (c) on the mask = 1 object of (a): mbavo_pairs_set_masks with geometry 0 (a copy and the clearance launches) and with geometry 1
      (the warp launch and the clearance launches), each up to a synchronisation, beside the camera call of the same object (the
      map launch and the clearance launches) and the camera call of an object with valid_radius = 0 (the map launch alone).
Recorded: the differences of the medians against the spreads of the same run, the keypoint counts per level, the launch statistics
and the device bytes of the objects.  Records, not gates.
Usage: python tools/pairs_mask_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r22_pairs_mask.txt), one JSON line per B at its end"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed
from pairs_valid_bench import RADIUS, TO_INTR


def bonnet(h, w):
    """0 inside a half-ellipse at the bottom of an h x w image, 255 outside."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = ((x - 0.5 * w) / (0.62 * w)) ** 2 + ((h - 1 - y) / (0.45 * h)) ** 2 <= 1.0
    return np.where(inside, 0, 255).astype(np.uint8)


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    sharp, blur, z = inputs(B)
    mask = torch.from_numpy(bonnet(H, W)[None]).to("cuda:0")  # (raw and undistorted images have one size here: one array serves both geometries)
    cam = workloads.camera_radtan(H, W, INTR, DIST)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "radius": RADIUS, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, one camera, bonnet mask over %.1f %% of the image, min / median / max of %d, interleaved:" % (
        B, L_LEVELS, W, H, 100.0 * float((mask == 0).float().mean()), reps))
    for dense in (False, True):
        make = lambda **kw: workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=4, N=4, intr=TO_INTR, cell=30, thresh=THRESH,
                                                every_candidate=dense, **kw)
        objs = {"a0": make(undistort=1, valid_radius=RADIUS), "a1": make(undistort=1, valid_radius=RADIUS, mask=1),
                "b0": make(undistort=0), "b1": make(undistort=0, valid_radius=RADIUS, mask=1), "c0": make(undistort=1)}
        for n in ("a0", "a1", "c0"):
            assert objs[n].set_camera(cam) == 0
        assert objs["a1"].set_masks(mask, 1) == 0 and objs["b1"].set_masks(mask, 0) == 0
        prep = ("a0", "a1", "b0", "b1")
        counts, ts = {}, {n: [] for n in prep}
        ways = {n: (lambda n=n: counts.__setitem__(n, objs[n].prepare(sharp, z, blur))) for n in prep}
        calls = {"set_masks geometry 0": lambda: objs["a1"].set_masks(mask, 0), "set_masks geometry 1": lambda: objs["a1"].set_masks(mask, 1),
                 "camera call, mask = 1": lambda: objs["a1"].set_camera(cam), "camera call, valid_radius = 2": lambda: objs["a0"].set_camera(cam),
                 "camera call, valid_radius = 0": lambda: objs["c0"].set_camera(cam)}
        cs = {n: [] for n in calls}
        for fn in list(ways.values()) + list(calls.values()):  # warm-up
            fn()
        for _ in range(reps):
            for n, fn in calls.items():
                cs[n].append(timed(lambda: (fn() == 0) or sys.exit("a call failed: " + n)))
            assert objs["a1"].set_masks(mask, 1) == 0  # (the route (a) object ends every round with the raw-geometry mask)
            for n, fn in ways.items():
                ts[n].append(timed(fn))
        med = {n: statistics.median(v) for n, v in ts.items()}
        spread = {n: max(v) - min(v) for n, v in ts.items()}
        cmed = {n: statistics.median(v) for n, v in cs.items()}
        name = "every candidate" if dense else "grid selection (cell 30)"
        rec = {"prepare_min_med_max_ms": {n: mmm(ts[n]) for n in prep}, "spread_ms": {n: round(v, 3) for n, v in spread.items()},
               "a_mask_minus_plain_median_ms": round(med["a1"] - med["a0"], 3), "b_mask_minus_plain_median_ms": round(med["b1"] - med["b0"], 3),
               "calls_min_med_max_ms": {n: mmm(v) for n, v in cs.items()}, "calls_spread_ms": {n: round(max(v) - min(v), 3) for n, v in cs.items()},
               "keypoints_per_level": {n: [int(v) for v in counts[n].sum(0)] for n in prep},
               "stats": {n: list(objs[n].stats()[:3]) for n in prep}, "object_bytes": {n: objs[n].stats()[3] for n in objs}}
        out["routes"][name] = rec
        emit("  %s" % name)
        for n, what in (("a0", "(a) undistort = 1, valid_radius = %d" % RADIUS), ("a1", "(a) the same, mask = 1, bonnet set"),
                        ("b0", "(b) undistort = 0, plain"), ("b1", "(b) undistort = 0, mask = 1, valid_radius = %d, bonnet set" % RADIUS)):
            emit("    %-58s %9.3f / %9.3f / %9.3f ms   spread %.3f ms; launches, synchronisations, D2H bytes %s; object %.1f MB; keypoints per level %s" % (
                (what,) + tuple(rec["prepare_min_med_max_ms"][n]) + (spread[n], rec["stats"][n], rec["object_bytes"][n] / 1e6, rec["keypoints_per_level"][n])))
        emit("    medians: (a) mask - plain = %.3f ms against spreads of %.3f / %.3f ms; (b) mask - plain = %.3f ms against spreads of %.3f / %.3f ms" % (
            med["a1"] - med["a0"], spread["a0"], spread["a1"], med["b1"] - med["b0"], spread["b0"], spread["b1"]))
        for n in calls:
            emit("    (c) %-32s to a synchronisation %s ms, spread %.3f ms" % (n, rec["calls_min_med_max_ms"][n], rec["calls_spread_ms"][n]))
        emit("    (c) medians over the map launch alone: set_masks geometry 0 %+.3f ms, geometry 1 %+.3f ms, camera call with mask = 1 %+.3f ms, "
             "camera call with valid_radius = 2 %+.3f ms" % tuple(cmed[n] - cmed["camera call, valid_radius = 0"] for n in list(calls)[:4]))
        for o in objs.values():
            o.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r22_pairs_mask.txt")
    Bs = [int(a) for a in rest] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(ctx, B, emit) for B in Bs]
    for r in results:
        emit(json.dumps(r))
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
