"""Every semi-dense candidate as a keypoint (mbavo_pairs_opts.every_candidate = 1) for a batch of rendered keyframe pairs
(640 x 480, 4 pyramid levels), two ways inside one process, interleaved, `reps` repetitions each after a warm-up, every repetition
ending in a device synchronisation:
  (a) mbavo_pairs_prepare: all pairs and levels in ceil((L-1)/3) + 4 launches and one stream synchronisation;
  (b) the B x L per-image call sequence it replaces: per pair two mbavo_pyramid_levels_u8, per pair and level one
      mbavo_image_gradients_u8, one mbavo_detect_semidense with cell 0 (3 launches, a copy and a synchronisation) and the border
      filter in torch.  Its output buffers are allocated once, outside the timing.
Checks that both ways find the same keypoint counts.  Then, from one profiled prepare (torch.profiler's kernel records), the time
of the three selection launches and their achieved bytes per second (keyframe image bytes read + keypoint bytes written, against
8 TB/s), and for the first B one mbavo_lm_batch_levels call on the dense array: ms per call, slots, us per slot, and the kernels
that take its time.
Usage: python tools/pairs_dense_bench.py [B ...]  (default 64 512)   -> profiles/r13_pairs_dense.txt, one JSON line per B at its end"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

L_LEVELS, THRESH, HBM_BYTES_PER_S = 4, 4.0, 8e12


def per_image_buffers(sharp, L):
    import torch
    B, H, W = sharp.shape
    dev = sharp.device
    out = []
    for b in range(B):
        lv = []
        for l in range(L):
            n = (H >> l) * (W >> l)
            lv.append(dict(ref=torch.empty(n, dtype=torch.uint8, device=dev) if l else None, cur=torch.empty(n, dtype=torch.uint8, device=dev) if l else None,
                           grad=torch.empty(2 * n, dtype=torch.float32, device=dev), xy=torch.empty(2 * n, dtype=torch.float64, device=dev),
                           z=torch.empty(n, dtype=torch.float64, device=dev)))
        out.append(lv)
    return out


def per_image(ctx, capi, sharp, depth, blur, L, bufs):
    """(b); the keypoint counts."""
    lib = ctx.lib
    B, H, W = sharp.shape
    counts = np.zeros((B, L), np.int32)
    keep = []
    for b in range(B):
        refs = [sharp[b].view(-1)] + [bufs[b][l]["ref"] for l in range(1, L)]
        curs = [blur[b].view(-1)] + [bufs[b][l]["cur"] for l in range(1, L)]
        for lv in (refs, curs):
            ptrs = (C.c_void_p * L)(*[a.data_ptr() for a in lv])
            capi.check(lib.mbavo_pyramid_levels_u8(ctx.handle, ptrs, H, W, L), "mbavo_pyramid_levels_u8")
        for l in range(L):
            Hl, Wl = H >> l, W >> l
            u = bufs[b][l]
            capi.check(lib.mbavo_image_gradients_u8(refs[l].data_ptr(), Hl, Wl, u["grad"].data_ptr(), None), "mbavo_image_gradients_u8")
            cnt = C.c_int(0)
            capi.check(lib.mbavo_detect_semidense(ctx.handle, refs[l].data_ptr(), Hl, Wl, l, H, W, 0, 0, THRESH, depth[b].data_ptr(),
                                                  u["xy"].data_ptr(), u["z"].data_ptr(), Hl * Wl, C.byref(cnt)), "mbavo_detect_semidense")
            K = cnt.value
            margin = max(4, 20 >> l)
            xyv = u["xy"][:2 * K].view(K, 2)
            ok = (xyv[:, 0] >= margin) & (xyv[:, 0] < Wl - margin) & (xyv[:, 1] >= margin) & (xyv[:, 1] < Hl - margin)
            xy, kz = xyv[ok].contiguous().view(-1), u["z"][:K][ok].contiguous()
            counts[b, l] = int(kz.shape[0])
            keep += [xy, kz]
    return counts


def kernel_times(fn):
    """{kernel name: (calls, total us)} of fn() by torch.profiler (empty where it records no kernels)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    out = {}
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        for ev in prof.events():
            if "k_" in ev.name:
                t = getattr(ev, "device_time", None)
                t = getattr(ev, "cuda_time", 0.0) if t is None else t
                n, s = out.get(ev.name, (0, 0.0))
                out[ev.name] = (n + 1, s + float(t))
    except Exception as exc:  # the figures are for the record; the timings above do not depend on them
        print("  (no kernel records: %s)" % exc)
    return out


def short(name):
    name = name.replace("void ", "").replace("mbavo::", "").replace("pairs::", "")
    return name.split("(")[0][:60]


def bench(M, ctx, B, emit, with_lm, reps=10, seed=1):
    import torch
    import lm_levels_bench
    from mba_vo_amd import workloads
    capi = M.capi
    L = L_LEVELS
    rpp = workloads.RenderedPairPyramids(ctx, B, L=L, S=8, k=4, seed=seed, thresh=THRESH)
    H, W = rpp.H, rpp.W
    sharp, depth, blur = workloads.rendered_inputs(rpp)
    out = {"B": B, "L": L, "H": H, "W": W, "reps": reps}
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=8, k=4, N=4, intr=rpp.intr, keyframe_format=0, cell=0, thresh=THRESH, every_candidate=True)
    bufs = per_image_buffers(sharp, L)
    ca = pb.prepare(sharp, depth, blur)  # warm-up, both ways
    cb = per_image(ctx, capi, sharp, depth, blur, L, bufs)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((lambda: pb.prepare(sharp, depth, blur), ta), (lambda: per_image(ctx, capi, sharp, depth, blur, L, bufs), tb)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t))
    launches, syncs, d2h, held = pb.stats()
    out.update(a_median_ms=round(statistics.median(ta), 3), a_min_ms=round(min(ta), 3), b_median_ms=round(statistics.median(tb), 3),
               b_min_ms=round(min(tb), 3), b_over_a_median=round(statistics.median(tb) / statistics.median(ta), 2),
               counts_equal=bool(np.array_equal(ca, cb)), launches=launches, synchronisations=syncs, d2h_bytes=d2h, device_bytes=held,
               K_per_level_mean=[round(float(ca[:, l].mean()), 1) for l in range(L)])
    emit("B = %d pairs, %d levels of %dx%d, median of %d, interleaved; %.2f GB held, keypoints per level (mean) %s:" % (
        B, L, W, H, reps, held / 1e9, out["K_per_level_mean"]))
    emit("  (a) mbavo_pairs_prepare, every_candidate = 1   median %9.3f ms  min %9.3f ms   %d launches, %d synchronisation, %d B D2H" % (
        out["a_median_ms"], out["a_min_ms"], launches, syncs, d2h))
    emit("  (b) per-image calls, %5d x %d levels          median %9.3f ms  min %9.3f ms   (b / a = %.2f on the medians; counts equal: %s)" % (
        B, L, out["b_median_ms"], out["b_min_ms"], out["b_over_a_median"], out["counts_equal"]))
    # the selection launches of one prepare
    kt = kernel_times(lambda: pb.prepare(sharp, depth, blur))
    sel = {short(k): v for k, v in kt.items() if "k_pairs_dense" in k}
    if sel:
        us = sum(v[1] for v in sel.values())
        px = B * sum((H >> l) * (W >> l) for l in range(L))
        nbytes = px + 24 * int(ca.sum())  # keyframe image bytes read (once) + keypoint bytes written
        out.update(selection_us=round(us, 1), selection_bytes=nbytes, selection_TB_per_s=round(nbytes / (us * 1e-6) / 1e12, 3),
                   selection_fraction_of_hbm=round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3))
        emit("  selection launches: %s" % ", ".join("%s %.1f us" % (k, v[1]) for k, v in sorted(sel.items())))
        emit("    %.1f us in all, %.1f MB (image bytes read once + 24 B per keypoint written): %.3f TB/s = %.3f of 8 TB/s" % (
            us, nbytes / 1e6, out["selection_TB_per_s"], out["selection_fraction_of_hbm"]))
        emit("    every kernel of the prepare: %s" % ", ".join("%s %.1f us" % (short(k), v[1]) for k, v in sorted(kt.items(), key=lambda kv: -kv[1][1])))
    if with_lm:
        pairs = [rpp.pair(b) for b in range(B)]
        motion = ([h.cap for h in pairs], [h.exp for h in pairs], [h.t0 for h in pairs], 0.5,
                  np.stack([h.kt for h in pairs]), np.stack([h.kR for h in pairs]))
        reset = lambda: capi.check(pb.set_motion(*motion), "mbavo_pairs_set_motion")
        reset()
        os.environ["MBAVO_LM_STAMPS"] = "1"
        try:
            slots = lm_levels_bench._slots(lm_levels_bench._stderr_of(lambda: lm_levels_bench.run_levels(M, ctx, pb, trace=False)))  # (also the warm-up)
        finally:
            del os.environ["MBAVO_LM_STAMPS"]
        ms = lm_levels_bench.best_ms(lambda: lm_levels_bench.run_levels(M, ctx, pb, trace=False), reset, 2)
        out.update(lm_batch_levels_ms=round(ms, 3), lm_slots=slots, lm_us_per_slot=round(1e3 * ms / max(slots, 1), 1))
        emit("  mbavo_lm_batch_levels on the dense array (S = 8, 8-pixel pattern, k = 4; best of 2): %.3f ms per call, %d slots, %.1f us per slot" % (
            ms, slots, out["lm_us_per_slot"]))
        reset()
        kt = kernel_times(lambda: lm_levels_bench.run_levels(M, ctx, pb, trace=False))
        tot = sum(v[1] for v in kt.values())
        if tot > 0:
            top = sorted(kt.items(), key=lambda kv: -kv[1][1])[:6]
            out["lm_kernels"] = {short(k): [v[0], round(v[1], 1)] for k, v in top}
            emit("    kernel time %.3f ms; by kernel: %s" % (tot / 1e3, ", ".join("%s x%d %.1f us (%.0f %%)" % (short(k), v[0], v[1], 100 * v[1] / tot) for k, v in top)))
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

    results = [bench(mbavo, ctx, B, emit, with_lm=(i == 0)) for i, B in enumerate(Bs)]
    for r in results:
        emit(json.dumps(r))
    with open(os.path.join(ROOT, "profiles", "r13_pairs_dense.txt"), "w") as f:
        f.write("\n".join(text) + "\n")
    ctx.close()
