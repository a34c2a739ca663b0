"""What reading ray-distance and 16-bit depth maps directly costs a batch of keyframe pairs (mbavo_pairs_opts.depth_format), at
640 x 480 with 4 pyramid levels, for grid selection and for every_candidate = 1.  Three ways inside one process, interleaved,
`reps` repetitions each after a warm-up, every repetition between two device synchronisations; min / median / max:
  (a) mbavo_pairs_prepare with depth_format 1 (ray distance, depth_max 100) and 2 (uint16, depth_unit 5000) on the raw maps;
  (b) mbavo_depth_to_z over the B maps (B launches, into a float buffer allocated once, outside the timing), then a format-0
      mbavo_pairs_prepare on the result; the conversion's share is also timed alone;
  (c) the format-0 mbavo_pairs_prepare alone, on the converted maps.
Checks that (a) and (b) find the same keypoint counts, and records the device bytes (b) needs on top of the object: the float
buffer, 4 B H W.  The maps are synthetic: z uniform in 0.5 .. 3 m with a tenth of the pixels without depth, stored as the distance
along the ray of a pinhole camera (fx = fy = cx = 320, cy = 240) and as uint16 of 1 / 5000 m; the images are rolled copies of eight
textures.
Usage: python tools/pairs_depth_bench.py [B ...]  (default 64 512)   -> profiles/r14_pairs_depth.txt, one JSON line per B at its end"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

L_LEVELS, H, W, THRESH = 4, 480, 640, 4.0
INTR = (W / 2.0, W / 2.0, W / 2.0, H / 2.0)
SETTINGS = {1: (0.0, 100.0), 2: (5000.0, 0.0)}  # depth_format: (depth_unit, depth_max)


def inputs(B, seed=1):
    """(sharp, blur) B x H x W uint8 and {format: raw maps} on the device."""
    import torch
    from mba_vo_amd import synth
    base = torch.from_numpy(np.stack([synth.texture_image(H, W, seed=seed + i, octaves=(32, 16, 8, 4)) for i in range(8)])).to("cuda:0")
    sharp = torch.stack([torch.roll(base[b % 8], (7 * (b // 8), 13 * (b // 8)), (0, 1)) for b in range(B)]).contiguous()
    blur = torch.roll(sharp, (1, 2), (1, 2)).contiguous()
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    z = torch.rand((B, H, W), generator=g, device="cuda:0", dtype=torch.float32) * 2.5 + 0.5
    z[torch.rand((B, H, W), generator=g, device="cuda:0") < 0.1] = 0.0
    xn = (torch.arange(W, device="cuda:0", dtype=torch.float64) - INTR[2]) / INTR[0]
    yn = (torch.arange(H, device="cuda:0", dtype=torch.float64) - INTR[3]) / INTR[1]
    n = torch.sqrt(xn[None, :] ** 2 + yn[:, None] ** 2 + 1.0)
    ray = (z.double() * n).float().contiguous()
    u16 = (z * 5000.0).round().clamp(0, 32767).to(torch.int16).contiguous()  # (below 2^15: int16 and uint16 hold the same bits)
    return sharp, blur, {1: ray, 2: u16}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def mmm(ts):
    return [round(min(ts), 3), round(statistics.median(ts), 3), round(max(ts), 3)]


def bench(M, ctx, B, dense, emit, reps=10):
    import torch
    from mba_vo_amd import workloads
    capi, lib = M.capi, ctx.lib
    sharp, blur, raw = inputs(B)
    K = np.array(INTR, np.float64)
    zbuf = torch.empty((B, H, W), dtype=torch.float32, device="cuda:0")  # what (b) needs on top of the object

    def convert(fmt):
        src, step = raw[fmt].data_ptr(), raw[fmt].element_size() * H * W
        unit, dmax = SETTINGS[fmt]
        for b in range(B):
            rc = lib.mbavo_depth_to_z(ctx.handle, fmt, src + b * step, H, W, capi.dp(K), unit, dmax, zbuf.data_ptr() + 4 * b * H * W)
            assert rc == 0, rc

    def batch(fmt):
        unit, dmax = SETTINGS.get(fmt, (0.0, 0.0))
        return workloads.PairBatch(ctx, B, L=L_LEVELS, H=H, W=W, S=8, k=4, N=4, intr=INTR, cell=0 if dense else 30, thresh=THRESH,
                                   every_candidate=dense, depth_format=fmt, depth_unit=unit, depth_max=dmax)

    pbs = {fmt: batch(fmt) for fmt in (0, 1, 2)}
    counts = {}
    ways = {}
    for fmt in (1, 2):
        ways["a%d" % fmt] = lambda fmt=fmt: counts.__setitem__(("a", fmt), pbs[fmt].prepare(sharp, raw[fmt], blur))
        ways["b%d" % fmt] = lambda fmt=fmt: (convert(fmt), counts.__setitem__(("b", fmt), pbs[0].prepare(sharp, zbuf, blur)))
        ways["conv%d" % fmt] = lambda fmt=fmt: convert(fmt)
    ways["c"] = lambda: pbs[0].prepare(sharp, zbuf, blur)
    ts = {name: [] for name in ways}
    for fn in ways.values():  # warm-up
        fn()
    for _ in range(reps):
        for name, fn in ways.items():
            ts[name].append(timed(fn))
    launches = {fmt: pbs[fmt].stats()[:3] for fmt in pbs}
    held = pbs[0].stats()[3]
    equal = all(np.array_equal(counts[("a", fmt)], counts[("b", fmt)]) for fmt in (1, 2))
    out = {"B": B, "L": L_LEVELS, "H": H, "W": W, "every_candidate": int(dense), "reps": reps, "counts_equal": bool(equal),
           "stats_per_format": {str(f): list(v) for f, v in launches.items()}, "object_bytes": held, "extra_bytes_b": 4 * B * H * W,
           "raw_bytes": {str(f): raw[f].numel() * raw[f].element_size() for f in raw},
           "keypoints_mean": [round(float(counts[("a", 1)][:, l].mean()), 1) for l in range(L_LEVELS)]}
    out.update({"%s_min_med_max_ms" % name: mmm(v) for name, v in ts.items()})
    emit("B = %d pairs, %d levels of %dx%d, %s, min / median / max of %d, interleaved; object %.2f GB for every format, keypoints per level (mean) %s:" % (
        B, L_LEVELS, W, H, "every_candidate = 1" if dense else "grid selection (cell 30)", reps, held / 1e9, out["keypoints_mean"]))
    label = {1: "ray distance, depth_max 100", 2: "uint16 / 5000"}
    for fmt in (1, 2):
        emit("  (a) prepare, depth_format %d (%s) on the raw maps      %9.3f / %9.3f / %9.3f ms   launches, synchronisations, D2H bytes %s" % (
            (fmt, label[fmt]) + tuple(out["a%d_min_med_max_ms" % fmt]) + (launches[fmt],)))
        emit("  (b) mbavo_depth_to_z x %d + format-0 prepare            %9.3f / %9.3f / %9.3f ms   (the %d conversions alone %9.3f / %9.3f / %9.3f ms; + %.1f MB)" % (
            (B,) + tuple(out["b%d_min_med_max_ms" % fmt]) + (B,) + tuple(out["conv%d_min_med_max_ms" % fmt]) + (4 * B * H * W / 1e6,)))
    emit("  (c) format-0 prepare alone on the converted maps         %9.3f / %9.3f / %9.3f ms   launches, synchronisations, D2H bytes %s" % (
        tuple(out["c_min_med_max_ms"]) + (launches[0],)))
    emit("  counts of (a) and (b) equal: %s; median a1 / c = %.3f, a2 / c = %.3f, b1 / c = %.3f, b2 / c = %.3f" % (
        equal, *[statistics.median(ts[n]) / statistics.median(ts["c"]) for n in ("a1", "a2", "b1", "b2")]))
    for pb in pbs.values():
        pb.close()
    return out


if __name__ == "__main__":
    import torch
    import mba_vo_amd as mbavo
    Bs = [int(a) for a in sys.argv[1:]] or [64, 512]
    ctx = mbavo.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    text = []

    def emit(line):
        print(line)
        sys.stdout.flush()
        text.append(line)

    results = [bench(mbavo, ctx, B, dense, emit) for B in Bs for dense in (False, True)]
    for r in results:
        emit(json.dumps(r))
    with open(os.path.join(ROOT, "profiles", "r14_pairs_depth.txt"), "w") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
