"""What the clearance mask of a batch of keyframe pairs costs (mbavo_pairs_opts.valid_radius), at 640 x 480 with 4 pyramid levels
and undistort = 1, under a `to` camera wide enough that the undistorted images have a black margin.  For one camera and for a set
of G = 4, for grid selection and for every candidate, inside one process, interleaved, `reps` repetitions each after a warm-up,
every repetition between two device synchronisations; min / median / max and the spread (max - min):
  (a) a mbavo_pairs_prepare with valid_radius = 0;
  (b) the same library and inputs with valid_radius = 2;
  (c) the camera call alone (mbavo_pairs_set_camera, or mbavo_pairs_set_cameras with G = 4) up to a synchronisation, on the
      object of (a) -- the map launch -- and on the object of (b) -- the map launch and the clearance stage behind it.
Recorded: (b) - (a) against the spread of (a), the extra time of (c), the keypoint counts of (a) and (b) per level, the launch
statistics and the device bytes of both objects.
Usage: python tools/pairs_valid_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r21_pairs_valid.txt), one JSON line per B at its end"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed

RADIUS = 2
TO_INTR = (0.62 * INTR[0], 0.62 * INTR[1], INTR[2], INTR[3])  # a wide view of the TUM-like raw camera: its corners are black


def camera_set(G):
    from mba_vo_amd import workloads
    raw = workloads.camera_radtan(H, W, INTR, DIST)
    scale = lambda g: 1.0 + 0.02 * g / max(G - 1, 1)
    return [workloads.pairs_camera(raw, (TO_INTR[0] * scale(g), TO_INTR[1] * scale(g), TO_INTR[2], TO_INTR[3])) for g in range(G)]


def bench(ctx, B, emit, reps=10):
    from mba_vo_amd import workloads
    sharp, blur, z = inputs(B)
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "radius": RADIUS, "routes": {}}
    emit("B = %d pairs, %d levels of %dx%d, undistort = 1, to_intrinsics = 0.62 x the raw focal length, valid_radius = %d against 0, "
         "min / median / max of %d, interleaved:" % (B, L_LEVELS, W, H, RADIUS, reps))
    for dense in (False, True):
        for G in (0, 4):
            objs = {n: workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=4, N=4, intr=TO_INTR, cell=30, thresh=THRESH, undistort=1,
                                           every_candidate=dense, num_cameras=G, valid_radius=r) for n, r in (("a", 0), ("b", RADIUS))}
            if G:
                cams, idx = camera_set(G), [b % G for b in range(B)]
                call = lambda o: o.set_cameras(cams, idx)
            else:
                cam = workloads.camera_radtan(H, W, INTR, DIST)
                call = lambda o: o.set_camera(cam)
            counts, ts, cs = {}, {n: [] for n in objs}, {n: [] for n in objs}
            ways = {n: (lambda n=n: counts.__setitem__(n, objs[n].prepare(sharp, z, blur))) for n in objs}
            for n, o in objs.items():  # warm-up
                assert call(o) == 0
                ways[n]()
            for _ in range(reps):
                for n, o in objs.items():
                    cs[n].append(timed(lambda: call(o)))
                for n, fn in ways.items():
                    ts[n].append(timed(fn))
            med = {n: statistics.median(v) for n, v in ts.items()}
            spread = {n: max(v) - min(v) for n, v in ts.items()}
            name = "%s, %s" % ("every candidate" if dense else "grid selection (cell 30)", "G = 4 cameras" if G else "one camera")
            rec = {"a_min_med_max_ms": mmm(ts["a"]), "b_min_med_max_ms": mmm(ts["b"]), "b_minus_a_median_ms": round(med["b"] - med["a"], 3),
                   "spread_ms": {n: round(v, 3) for n, v in spread.items()},
                   "camera_call_a_min_med_max_ms": mmm(cs["a"]), "camera_call_b_min_med_max_ms": mmm(cs["b"]),
                   "camera_call_b_minus_a_median_ms": round(statistics.median(cs["b"]) - statistics.median(cs["a"]), 3),
                   "keypoints_per_level": {n: [int(v) for v in counts[n].sum(0)] for n in objs},
                   "stats": {n: list(o.stats()[:3]) for n, o in objs.items()}, "object_bytes": {n: o.stats()[3] for n, o in objs.items()}}
            out["routes"][name] = rec
            emit("  %s" % name)
            for n, what in (("a", "valid_radius = 0"), ("b", "valid_radius = %d" % RADIUS)):
                emit("    (%s) prepare, %-17s %9.3f / %9.3f / %9.3f ms   spread %.3f ms; launches, synchronisations, D2H bytes %s; object %.1f MB; "
                     "keypoints per level %s" % ((n, what) + tuple(rec["%s_min_med_max_ms" % n]) + (spread[n], rec["stats"][n],
                                                                                                      rec["object_bytes"][n] / 1e6, rec["keypoints_per_level"][n])))
            emit("    medians: (b) - (a) = %.3f ms against a spread of (a) of %.3f ms" % (med["b"] - med["a"], spread["a"]))
            emit("    (c) camera call to a synchronisation: without the clearance stage %s ms, with it %s ms, medians differ by %.3f ms" % (
                rec["camera_call_a_min_med_max_ms"], rec["camera_call_b_min_med_max_ms"], rec["camera_call_b_minus_a_median_ms"]))
            for o in objs.values():
                o.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r21_pairs_valid.txt")
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
