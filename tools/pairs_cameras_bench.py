"""What a set of cameras in one batch of keyframe pairs costs (mbavo_pairs_opts.num_cameras, mbavo_pairs_set_cameras), at
640 x 480 with 4 pyramid levels, grid selection and undistort = 1.  Four routes inside one process, interleaved, `reps`
repetitions each after a warm-up, every repetition a mbavo_pairs_prepare between two device synchronisations; min / median / max
and the spread (max - min):
  (a) one camera for all pairs (num_cameras = 0, mbavo_pairs_set_camera): the route that existed;
  (b) G = 4 cameras, pair b looks through camera b % 4;
  (c) G = B cameras, one per pair: B maps of 2.46 MB are read where (a) reads one;
  (c') as (c) on an object created under MBAVO_PAIRS_REMAP_BOTH=0: the remap of a prepare in 2B grid rows, one image each, every
      map read twice, where (c) remaps both images of a pair in one lane from one read of the map entries.
The G cameras are the TUM-like radial-tangential camera of tools/pairs_undistort_bench.py with the focal length of `to_intrinsics`
changed by up to 2 % from camera to camera, so that every map differs.  Checks that (b) and (c) give the pairs of camera 0 the
keypoint counts (a) gives them, and records the device bytes of each object and the cost of set_cameras itself.
Usage: python tools/pairs_cameras_bench.py [B ...] [OUT.txt]  (default 64 512)
   -> OUT.txt (a last argument that is no number; default profiles/r19_pairs_cameras.txt), one JSON line per B at its end
The one-camera route against the parent commit's library is tools/pairs_cameras_ab.py, which appends to the same file."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from pairs_undistort_bench import DIST, H, INTR, L_LEVELS, THRESH, W, inputs, mmm, timed


def camera_set(G):
    from mba_vo_amd import workloads
    raw = workloads.camera_radtan(H, W, INTR, DIST)
    scale = lambda g: 1.0 + 0.02 * g / max(G - 1, 1)
    return [workloads.pairs_camera(raw, (INTR[0] * scale(g), INTR[1] * scale(g), INTR[2], INTR[3])) for g in range(G)]


def bench(ctx, B, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    sharp, blur, z = inputs(B)

    def batch(G):
        return workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=4, N=4, intr=INTR, cell=30, thresh=THRESH, undistort=1, num_cameras=G)

    objs = {"a": batch(0), "b": batch(4), "c": batch(B)}
    os.environ["MBAVO_PAIRS_REMAP_BOTH"] = "0"  # (the library scans the environment on mbavo_reload_env; create reads the switch)
    ctx.lib.mbavo_reload_env()
    objs["c'"] = batch(B)
    del os.environ["MBAVO_PAIRS_REMAP_BOTH"]
    ctx.lib.mbavo_reload_env()
    assert objs["a"].set_camera(workloads.camera_radtan(H, W, INTR, DIST)) == 0
    set_ms = {}
    for name, G in (("b", 4), ("c", B), ("c'", B)):
        cams, idx = camera_set(G), [b % G for b in range(B)]
        assert objs[name].set_cameras(cams, idx) == 0
        set_ms[name] = mmm([timed(lambda: objs[name].set_cameras(cams, idx)) for _ in range(reps)])
    counts = {}
    ways = {name: (lambda name=name: counts.__setitem__(name, objs[name].prepare(sharp, z, blur))) for name in objs}
    ts = {name: [] for name in ways}
    for fn in ways.values():  # warm-up
        fn()
    for _ in range(reps):
        for name, fn in ways.items():
            ts[name].append(timed(fn))
    med = {n: statistics.median(v) for n, v in ts.items()}
    spread = {n: max(v) - min(v) for n, v in ts.items()}
    cam0 = {"b": list(range(0, B, 4)), "c": [0], "c'": [0]}
    equal = {n: bool(np.array_equal(counts[n][cam0[n]], counts["a"][cam0[n]])) for n in ("b", "c", "c'")}
    equal["c' = c"] = bool(np.array_equal(counts["c"], counts["c'"]))
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "counts_of_camera_0_equal": equal,
           "b_minus_a_median_ms": round(med["b"] - med["a"], 3), "c_minus_a_median_ms": round(med["c"] - med["a"], 3),
           "c1_minus_c_median_ms": round(med["c'"] - med["c"], 3),
           "spread_ms": {n: round(v, 3) for n, v in spread.items()}, "stats": {n: list(o.stats()[:3]) for n, o in objs.items()},
           "object_bytes": {n: o.stats()[3] for n, o in objs.items()}, "set_cameras_min_med_max_ms": set_ms}
    out.update({"%s_min_med_max_ms" % n: mmm(v) for n, v in ts.items()})
    emit("B = %d pairs, %d levels of %dx%d, grid selection (cell 30), undistort = 1, min / median / max of %d, interleaved:" % (B, L_LEVELS, W, H, reps))
    for n, what in (("a", "one camera (num_cameras = 0)"), ("b", "G = 4 cameras"), ("c", "G = B = %d cameras" % B), ("c'", "G = B, two rows per pair")):
        emit("  (%s) prepare, %-28s %9.3f / %9.3f / %9.3f ms   spread %.3f ms; launches, synchronisations, D2H bytes %s; object %.1f MB" % (
            (n, what) + tuple(out["%s_min_med_max_ms" % n]) + (spread[n], out["stats"][n], out["object_bytes"][n] / 1e6)))
    emit("  medians: (b) - (a) = %.3f ms, (c) - (a) = %.3f ms, (c') - (c) = %.3f ms; counts of camera 0's pairs equal to (a)'s, and (c') to (c): %s" % (
        med["b"] - med["a"], med["c"] - med["a"], med["c'"] - med["c"], equal))
    emit("  set_cameras (one copy, one launch over G maps, then a synchronisation of the timer's): G = 4 %s ms, G = %d %s ms" % (set_ms["b"], B, set_ms["c"]))
    for o in objs.values():
        o.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    rest = sys.argv[1:]
    out_path = rest.pop() if rest and not rest[-1].isdigit() else os.path.join(ROOT, "profiles", "r19_pairs_cameras.txt")
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
