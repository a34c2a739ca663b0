"""What keypoints from the caller cost in a batch of keyframe pairs (mbavo_pairs_prepare_points, _update_points) beside the detector
route, at 640 x 480 with 4 pyramid levels, on grid objects (cell 30) and on every_candidate = 1 objects.  Inside one process,
interleaved, `reps` repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max and
the spread (max - min):
  (a) mbavo_pairs_prepare (detector, float z maps) against mbavo_pairs_prepare_points on a second object of the same options; the
      points are the detector's own level-0 keypoints, cut to the smallest capacity over the levels (a longer row is
      MBAVO_E_RANGE: 63 with the grid, 60 x 80 = 4800 with every candidate);
  (b) an update with every second keyframe new, both ways;
  (c) one long list of 50 000 points per pair on an every_candidate = 1 object -- with L = 2 (capacity 240 x 320 = 76 800): at L = 4
      the smallest capacity is 4800 and such a row is rejected.  One workgroup per (pair, level) walks the list.
The library calls are timed alone: offsets and flat device arrays are built before the clock starts.  Records, not gates.
Usage: python tools/pairs_points_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r23_pairs_points.txt), one JSON line per B at its end"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_undistort_bench import H, L_LEVELS, THRESH, W, inputs, mmm, timed

LONG, LONG_LEVELS = 50000, 2


def level0_keypoints(pb, counts):
    """[(xy K x 2, z K)] per pair: level 0 of what the object holds, read through its problem array."""
    import torch
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    out = []
    for b in range(pb.B):
        q, K = pb.array[b * pb.L], int(counts[b, 0])
        xy, z = np.empty((K, 2)), np.empty(K)
        if K:
            assert hip.hipMemcpy(xy.ctypes.data, C.c_void_p(q.d_kp_xy), xy.nbytes, 2) == 0 and hip.hipMemcpy(z.ctypes.data, C.c_void_p(q.d_kp_z), z.nbytes, 2) == 0
        out.append((xy, z))
    return out


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import capi, workloads
    lib = ctx.lib
    sharp, blur, z = inputs(B)
    keys = np.arange(0, B, 2, dtype=np.int32)
    key_sharp, key_z = sharp[::2].contiguous(), z[::2].contiguous()
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, min / median / max of %d, interleaved:" % (B, L_LEVELS, W, H, reps))
    for dense in (False, True):
        make = lambda L=L_LEVELS: workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=8, k=4, N=4, cell=30, thresh=THRESH, every_candidate=dense)
        det, pts = make(), make()
        cells = (C.c_int * 8)()
        assert lib.mbavo_pairs_plan(C.byref(det.opts), C.byref(C.c_longlong(0)), cells) == 0
        cap = min(cells[:L_LEVELS])
        found = level0_keypoints(det, det.prepare(sharp, z, blur))
        lists = [(xy[:cap], zz[:cap]) for xy, zz in found]
        off, dxy, dz = pts._point_lists(lists, B)
        koff, kxy, kz = pts._point_lists(lists[::2], len(keys))
        counts_d, counts_p = np.zeros((B, L_LEVELS), np.int32), np.zeros((B, L_LEVELS), np.int32)
        ways = {
            "prepare, detector": lambda: lib.mbavo_pairs_prepare(det.handle, sharp.data_ptr(), z.data_ptr(), blur.data_ptr(), capi.ip(counts_d)),
            "prepare_points": lambda: lib.mbavo_pairs_prepare_points(pts.handle, sharp.data_ptr(), blur.data_ptr(), capi.ip(off), dxy.data_ptr(), dz.data_ptr(), capi.ip(counts_p)),
            "update, detector": lambda: lib.mbavo_pairs_update(det.handle, blur.data_ptr(), len(keys), capi.ip(keys), key_sharp.data_ptr(), key_z.data_ptr(), None),
            "update_points": lambda: lib.mbavo_pairs_update_points(pts.handle, blur.data_ptr(), len(keys), capi.ip(keys), key_sharp.data_ptr(), capi.ip(koff), kxy.data_ptr(), kz.data_ptr(), None),
        }
        ts = {n: [] for n in ways}
        for n, fn in ways.items():  # warm-up
            assert fn() == 0, n
        stats = {"prepare, detector": det.stats()[:3], "prepare_points": pts.stats()[:3], "update, detector": det.step_stats()[0], "update_points": pts.step_stats()[0]}
        for _ in range(reps):
            for n, fn in ways.items():
                ts[n].append(timed(lambda: fn() == 0 or sys.exit("a call failed: " + n)))
        med = {n: statistics.median(v) for n, v in ts.items()}
        spread = {n: max(v) - min(v) for n, v in ts.items()}
        name = "every candidate" if dense else "grid selection (cell 30)"
        rec = {"min_med_max_ms": {n: mmm(v) for n, v in ts.items()}, "spread_ms": {n: round(v, 3) for n, v in spread.items()},
               "stats": {n: [int(v) for v in s] for n, s in stats.items()}, "row_capacity": int(cap), "points_per_pair_median": int(np.median([len(l[1]) for l in lists])),
               "keypoints_per_level": {"detector": [int(v) for v in counts_d.sum(0)], "points": [int(v) for v in counts_p.sum(0)]},
               "prepare_points_minus_detector_median_ms": round(med["prepare_points"] - med["prepare, detector"], 3),
               "update_points_minus_detector_median_ms": round(med["update_points"] - med["update, detector"], 3)}
        emit("  %s: rows cut to the smallest capacity %d (median list %d points); keypoints per level: detector %s, points %s" % (
            name, cap, rec["points_per_pair_median"], rec["keypoints_per_level"]["detector"], rec["keypoints_per_level"]["points"]))
        for n in ways:
            emit("    %-20s %9.3f / %9.3f / %9.3f ms   spread %.3f ms; launches, synchronisations, D2H bytes %s" % ((n,) + tuple(rec["min_med_max_ms"][n]) + (spread[n], rec["stats"][n])))
        emit("    medians: prepare_points - detector prepare = %+.3f ms (spreads %.3f / %.3f ms); update_points - detector update = %+.3f ms (spreads %.3f / %.3f ms)" % (
            rec["prepare_points_minus_detector_median_ms"], spread["prepare_points"], spread["prepare, detector"],
            rec["update_points_minus_detector_median_ms"], spread["update_points"], spread["update, detector"]))
        det.close()
        pts.close()
        if dense:  # (c) the long list
            rng = np.random.default_rng(2)
            one = (np.stack([rng.uniform(0, W, LONG), rng.uniform(0, H, LONG)], 1), rng.uniform(0.5, 3.0, LONG))
            long_pb, short_pb = make(LONG_LEVELS), make(LONG_LEVELS)
            loff, lxy, lz = long_pb._point_lists([one] * B, B)
            soff, sxy, sz = short_pb._point_lists([(one[0][:256], one[1][:256])] * B, B)
            lw = {"50 000 points per pair": lambda: lib.mbavo_pairs_prepare_points(long_pb.handle, sharp.data_ptr(), blur.data_ptr(), capi.ip(loff), lxy.data_ptr(), lz.data_ptr(), None),
                  "256 points per pair": lambda: lib.mbavo_pairs_prepare_points(short_pb.handle, sharp.data_ptr(), blur.data_ptr(), capi.ip(soff), sxy.data_ptr(), sz.data_ptr(), None)}
            lt = {n: [] for n in lw}
            for n, fn in lw.items():
                assert fn() == 0, n
            for _ in range(reps):
                for n, fn in lw.items():
                    lt[n].append(timed(lambda: fn() == 0 or sys.exit("a call failed: " + n)))
            rec["long_list"] = {"L": LONG_LEVELS, "min_med_max_ms": {n: mmm(v) for n, v in lt.items()}, "spread_ms": {n: round(max(v) - min(v), 3) for n, v in lt.items()}}
            for n in lw:
                emit("    (c) L = %d, prepare_points with %-24s %9.3f / %9.3f / %9.3f ms   spread %.3f ms" % ((LONG_LEVELS, n) + tuple(rec["long_list"]["min_med_max_ms"][n]) + (rec["long_list"]["spread_ms"][n],)))
            emit("    (c) medians: the long lists cost %+.3f ms over the short ones (%d x %d x 24 bytes read, one workgroup per (pair, level))" % (
                statistics.median(lt["50 000 points per pair"]) - statistics.median(lt["256 points per pair"]), B, LONG))
            long_pb.close()
            short_pb.close()
        out["routes"][name] = rec
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r23_pairs_points.txt")
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
