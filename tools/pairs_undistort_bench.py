"""What undistorting the camera images inside a batch of keyframe pairs costs (mbavo_pairs_opts.undistort = 1), at 640 x 480 with 4
pyramid levels and grid selection.  Four routes inside one process, interleaved, `reps` repetitions each after a warm-up, every
repetition between two device synchronisations; min / median / max:
  (a) mbavo_pairs_prepare with undistort = 1 on the raw images (one remap launch in place of the two level-0 copies);
  (b) mbavo_undistort_u8 over the 2B raw images (2B launches, into a second buffer allocated once, outside the timing), then a
      plain mbavo_pairs_prepare on the result; the remap's share is also timed alone;
  (c) the plain mbavo_pairs_prepare alone, on the images (b) made;
  (d) ONE mbavo_undistort_u8_batch over the 2B raw images into that second buffer, then the plain mbavo_pairs_prepare; the one
      launch's share is also timed alone.  (d) is judged against (b) of the same run.
Checks that (a), (b) and (d) find the same keypoint counts, and records the device bytes each route needs on top of a plain object: the
one map for (a), the map and the second 2 B H W image buffer for (b).  The raw camera is a TUM-like one (640 x 480, fx 517.3,
fy 516.5, cx 318.6, cy 255.3, k1 k2 p1 p2 = 0.2624 -0.9531 -0.0054 0.0026), undistorted into a pinhole camera of the same size and
intrinsics; with --unified a unified camera instead (xi = 1, twice the focal length, k1 k2 p1 p2 = -0.05 0.01 0.0002 -0.0001:
the centre of the image keeps its scale), whose map mbavo_undistort_map_unified / mbavo_pairs_set_camera_unified make -- the routes
themselves do not know the camera model.  The images are rolled copies of eight textures, the depth maps z uniform in 0.5 .. 3 m with a tenth missing.
Usage: python tools/pairs_undistort_bench.py [--unified] [B ...]  (default 64 512)
   -> profiles/r18_pairs_undistort.txt (--unified: r18_pairs_undistort_unified.txt), one JSON line per B at its end"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

L_LEVELS, H, W, THRESH = 4, 480, 640, 4.0
INTR = (517.3, 516.5, 318.6, 255.3)
DIST = (0.2624, -0.9531, -0.0054, 0.0026)
UNIFIED_INTR, UNIFIED_XI, UNIFIED_DIST = (2 * 517.3, 2 * 516.5, 318.6, 255.3), 1.0, (-0.05, 0.01, 0.0002, -0.0001)


def inputs(B, seed=1):
    """(sharp, blur) B x H x W uint8 raw images and B x H x W float32 z maps on the device."""
    import torch
    from mba_vo_amd import synth
    base = torch.from_numpy(np.stack([synth.texture_image(H, W, seed=seed + i, octaves=(32, 16, 8, 4)) for i in range(8)])).to("cuda:0")
    sharp = torch.stack([torch.roll(base[b % 8], (7 * (b // 8), 13 * (b // 8)), (0, 1)) for b in range(B)]).contiguous()
    blur = torch.roll(sharp, (1, 2), (1, 2)).contiguous()
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    z = torch.rand((B, H, W), generator=g, device="cuda:0", dtype=torch.float32) * 2.5 + 0.5
    z[torch.rand((B, H, W), generator=g, device="cuda:0") < 0.1] = 0.0
    return sharp, blur, z


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def mmm(ts):
    return [round(min(ts), 3), round(statistics.median(ts), 3), round(max(ts), 3)]


def bench(M, ctx, B, emit, reps=10, unified=False):
    import torch
    from mba_vo_amd import workloads
    lib = ctx.lib
    sharp, blur, z = inputs(B)
    raw2 = torch.stack([sharp, blur])  # the 2B raw images in one buffer, for the one call of (d)
    sharp, blur = raw2[0], raw2[1]
    cam = workloads.camera_unified(H, W, UNIFIED_INTR, UNIFIED_XI, UNIFIED_DIST) if unified else workloads.camera_radtan(H, W, INTR, DIST)
    map_xy = workloads.undistort_map(ctx, cam, INTR, H, W)
    und = torch.empty((2, B, H, W), dtype=torch.uint8, device="cuda:0")  # what (b) needs on top of the object and the map

    def remap_all():
        for i, src in enumerate((sharp, blur)):
            for b in range(B):
                rc = lib.mbavo_undistort_u8(ctx.handle, src[b].data_ptr(), H, W, map_xy.data_ptr(), H, W, und[i, b].data_ptr())
                assert rc == 0, rc

    def remap_batch():
        rc = lib.mbavo_undistort_u8_batch(ctx.handle, raw2.data_ptr(), 2 * B, H, W, map_xy.data_ptr(), H, W, und.data_ptr())
        assert rc == 0, rc

    def batch(undistort):
        return workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=4, N=4, intr=INTR, cell=30, thresh=THRESH, undistort=undistort)

    fused, plain = batch(1), batch(0)
    assert fused.set_camera(cam) == 0
    counts = {}
    ways = {"a": lambda: counts.__setitem__("a", fused.prepare(sharp, z, blur)),
            "b": lambda: (remap_all(), counts.__setitem__("b", plain.prepare(und[0], z, und[1]))),
            "remap": remap_all,
            "c": lambda: plain.prepare(und[0], z, und[1]),
            "d": lambda: (remap_batch(), counts.__setitem__("d", plain.prepare(und[0], z, und[1]))),
            "remap_batch": remap_batch}
    ts = {name: [] for name in ways}
    for fn in ways.values():  # warm-up
        fn()
    for _ in range(reps):
        for name, fn in ways.items():
            ts[name].append(timed(fn))
    equal = bool(np.array_equal(counts["a"], counts["b"]))
    equal_d = bool(np.array_equal(counts["a"], counts["d"]))
    med = {n: statistics.median(v) for n, v in ts.items()}
    out = {"camera": "unified" if unified else "radtan", "counts_equal_d": equal_d, "d_minus_a_median_ms": round(med["d"] - med["a"], 3),
           "b_minus_d_median_ms": round(med["b"] - med["d"], 3), "B": B, "L": L_LEVELS, "H": H, "W": W, "reps": reps, "counts_equal": equal, "stats_fused": list(fused.stats()[:3]),
           "stats_plain": list(plain.stats()[:3]), "object_bytes_fused": fused.stats()[3], "object_bytes_plain": plain.stats()[3],
           "extra_bytes_b": int(und.numel() + map_xy.numel() * 4), "a_minus_c_median_ms": round(med["a"] - med["c"], 3),
           "b_minus_a_median_ms": round(med["b"] - med["a"], 3),
           "keypoints_mean": [round(float(counts["a"][:, l].mean()), 1) for l in range(L_LEVELS)]}
    out.update({"%s_min_med_max_ms" % name: mmm(v) for name, v in ts.items()})
    emit("B = %d pairs, %d levels of %dx%d, grid selection (cell 30), min / median / max of %d, interleaved; keypoints per level (mean) %s:" % (
        B, L_LEVELS, W, H, reps, out["keypoints_mean"]))
    emit("  (a) prepare, undistort = 1, on the raw images                %9.3f / %9.3f / %9.3f ms   launches, synchronisations, D2H bytes %s; object + %.1f MB (the map)" % (
        tuple(out["a_min_med_max_ms"]) + (out["stats_fused"], (out["object_bytes_fused"] - out["object_bytes_plain"]) / 1e6)))
    emit("  (b) mbavo_undistort_u8 x %4d + plain prepare                %9.3f / %9.3f / %9.3f ms   (the %d remaps alone %9.3f / %9.3f / %9.3f ms; + %.1f MB)" % (
        (2 * B,) + tuple(out["b_min_med_max_ms"]) + (2 * B,) + tuple(out["remap_min_med_max_ms"]) + (out["extra_bytes_b"] / 1e6,)))
    emit("  (c) plain prepare alone on the remapped images               %9.3f / %9.3f / %9.3f ms   launches, synchronisations, D2H bytes %s" % (
        tuple(out["c_min_med_max_ms"]) + (out["stats_plain"],)))
    emit("  counts of (a) and (b) equal: %s; medians: (a) - (c) = %.3f ms, (b) - (a) = %.3f ms; spread (max - min) of a / b / c: %.3f / %.3f / %.3f ms" % (
        equal, med["a"] - med["c"], med["b"] - med["a"], *[max(ts[n]) - min(ts[n]) for n in ("a", "b", "c")]))
    emit("  (d) mbavo_undistort_u8_batch (n = %4d) + plain prepare      %9.3f / %9.3f / %9.3f ms   (the one launch alone %9.3f / %9.3f / %9.3f ms)" % (
        (2 * B,) + tuple(out["d_min_med_max_ms"]) + tuple(out["remap_batch_min_med_max_ms"])))
    emit("  counts of (a) and (d) equal: %s; medians: (d) - (a) = %.3f ms, (b) - (d) = %.3f ms; spread (max - min) of d: %.3f ms; %s camera" % (
        equal_d, med["d"] - med["a"], med["b"] - med["d"], max(ts["d"]) - min(ts["d"]), out["camera"]))
    fused.close()
    plain.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    unified = "--unified" in sys.argv[1:]
    Bs = [int(a) for a in sys.argv[1:] if a != "--unified"] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(mbavo, ctx, B, emit, unified=unified) for B in Bs]
    for r in results:
        emit(json.dumps(r))
    with open(os.path.join(ROOT, "profiles", "r18_pairs_undistort_unified.txt" if unified else "r18_pairs_undistort.txt"), "w") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
