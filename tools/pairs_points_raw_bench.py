"""What the caller's points cost in the raw camera's geometry (mbavo_pairs_set_points_geometry(1)) beside the same points in the
undistorted geometry, on the workload of tools/pairs_points_bench.py: 640 x 480 x 4 levels, undistort = 1 (the TUM-like
radial-tangential camera of tools/pairs_undistort_bench.py), every_candidate = 1 objects.  The raw points are the detector's own
level-0 keypoints pushed through the forward map (the map entry of each keypoint's pixel), cut to the row capacity 4800; then one
list of 50 000 raw points per pair, uniform over the raw image (L = 2, as in pairs_points_bench.py).  Inside one process,
interleaved, `reps` repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max and
the spread (max - min):
  (1) mbavo_pairs_prepare_points in geometry 1 on the raw points -- the inverse camera inside the points kernel, once per level;
  (0) mbavo_pairs_prepare_points in geometry 0 on the undistorted points -- no inverse at all;
  (c) mbavo_undistort_points_batch (one row per pair) into a buffer allocated once, then (0) on its output -- the inverse once per
      point, 32 bytes more traffic per point; the stand-alone launch is also timed alone.
(1) - (0) is what the L inversions of a point cost on top of the kernel's memory traffic, (c) - (1) what fusing saves or loses.
The library calls are timed alone: offsets and flat device arrays are built before the clock starts.  Records, not gates.
Usage: python tools/pairs_points_raw_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> appended to OUT.txt (a last argument that is no number; default profiles/r29_pairs_points_raw.txt), one JSON line per B"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_points_bench import LONG, LONG_LEVELS, level0_keypoints
from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import capi, workloads
    lib = ctx.lib
    sharp, blur, z = inputs(B)
    cam = workloads.camera_radtan(H, W, INTR, DIST)
    cams = (capi.PairsCamera * B)(*([workloads.pairs_camera(cam, INTR)] * B))
    map_xy = workloads.undistort_map(ctx, cam, INTR, H, W)
    torch.cuda.synchronize()
    map_xy = map_xy.cpu().numpy().astype(np.float64)

    def make(L=L_LEVELS):
        pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=8, k=4, N=4, intr=INTR, cell=30, thresh=THRESH, every_candidate=True, undistort=1)
        assert pb.set_camera(cam) == 0
        return pb

    out = {"B": B, "H": H, "W": W, "reps": reps, "workloads": {}}
    emit("B = %d pairs, %dx%d, undistort = 1, every candidate, min / median / max of %d, interleaved:" % (B, W, H, reps))
    det = make()
    cells = (C.c_int * 8)()
    assert lib.mbavo_pairs_plan(C.byref(det.opts), C.byref(C.c_longlong(0)), cells) == 0
    cap = min(cells[:L_LEVELS])
    found = [(xy[:cap], zz[:cap]) for xy, zz in level0_keypoints(det, det.prepare(sharp, z, blur))]
    det.close()
    through_map = [(map_xy[xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)], zz) for xy, zz in found]
    rng = np.random.default_rng(2)
    long_raw = (np.stack([rng.uniform(0, W - 1, LONG), rng.uniform(0, H - 1, LONG)], 1), rng.uniform(0.5, 3.0, LONG))
    for name, L, raw_lists, und_lists in (("the detector's keypoints through the map, rows cut to %d" % cap, L_LEVELS, through_map, found),
                                          ("%d raw points per pair" % LONG, LONG_LEVELS, [long_raw] * B, None)):
        raw_pb, und_pb = make(L), make(L)
        assert raw_pb.set_points_geometry(1) == 0
        off, d_uv, d_z = raw_pb._point_lists(raw_lists, B)
        d_tmp = torch.empty_like(d_uv)
        inverse = lambda: lib.mbavo_undistort_points_batch(ctx.handle, B, cams, capi.ip(off), d_uv.data_ptr(), d_tmp.data_ptr(), None)
        assert inverse() == 0
        if und_lists is None:  # the long list has no undistorted twin: geometry 0 runs on the inverse's output
            torch.cuda.synchronize()
            d_xy0 = d_tmp.clone()
        else:
            d_xy0 = und_pb._point_lists(und_lists, B)[1]
        c1, c0, cc = (np.zeros((B, L), np.int32) for _ in range(3))
        points = lambda pb, xy, counts: lib.mbavo_pairs_prepare_points(pb.handle, sharp.data_ptr(), blur.data_ptr(), capi.ip(off), xy.data_ptr(), d_z.data_ptr(), capi.ip(counts))
        ways = {"(1) geometry 1": lambda: points(raw_pb, d_uv, c1),
                "(0) geometry 0": lambda: points(und_pb, d_xy0, c0),
                "(c) inverse + geometry 0": lambda: inverse() or points(und_pb, d_tmp, cc),
                "    the inverse alone": inverse}
        ts = {n: [] for n in ways}
        for n, fn in ways.items():  # warm-up
            assert fn() == 0, n
        stats = {"(1) geometry 1": raw_pb.stats()[:3], "(0) geometry 0": und_pb.stats()[:3]}
        for _ in range(reps):
            for n, fn in ways.items():
                ts[n].append(timed(lambda: fn() == 0 or sys.exit("a call failed: " + n)))
        med = {n: statistics.median(v) for n, v in ts.items()}
        spread = {n: max(v) - min(v) for n, v in ts.items()}
        total = int(off[-1])
        rec = {"L": L, "points": total, "min_med_max_ms": {n.strip(): mmm(v) for n, v in ts.items()}, "spread_ms": {n.strip(): round(v, 3) for n, v in spread.items()},
               "stats": {n: [int(v) for v in s] for n, s in stats.items()}, "counts_fused_equal_composed": bool(np.array_equal(c1, cc)),
               "keypoints_per_level": {"geometry 1": [int(v) for v in c1.sum(0)], "geometry 0": [int(v) for v in c0.sum(0)]},
               "fused_minus_geometry0_median_ms": round(med["(1) geometry 1"] - med["(0) geometry 0"], 3),
               "composed_minus_fused_median_ms": round(med["(c) inverse + geometry 0"] - med["(1) geometry 1"], 3)}
        emit("  %s (L = %d, %d points in all); keypoints per level: geometry 1 %s, geometry 0 %s; fused and composed counts equal: %s" % (
            name, L, total, rec["keypoints_per_level"]["geometry 1"], rec["keypoints_per_level"]["geometry 0"], rec["counts_fused_equal_composed"]))
        for n in ways:
            emit("    %-26s %9.3f / %9.3f / %9.3f ms   spread %.3f ms%s" % ((n,) + tuple(mmm(ts[n])) + (spread[n], "; launches, synchronisations, D2H bytes %s" % rec["stats"][n] if n in stats else "")))
        emit("    medians: (1) - (0) = %+.3f ms for %d inversions of %d points (%d levels); (c) - (1) = %+.3f ms" % (
            rec["fused_minus_geometry0_median_ms"], L * total, total, L, rec["composed_minus_fused_median_ms"]))
        raw_pb.close()
        und_pb.close()
        out["workloads"][name] = rec
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r29_pairs_points_raw.txt")
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
    with open(out_path, "a") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
