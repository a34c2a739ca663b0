"""Where the pose PROLOGUE of k_fused<.., POSE> spends its time (library built with -DMBAVO_FUSED_STAMPS -DMBAVO_POSE_STAMPS:
bash tools/ab_build.sh pstamps "-DMBAVO_FUSED_STAMPS -DMBAVO_POSE_STAMPS"; cp tools/_ab/libmbavo_pstamps.so mba-vo_amd/libmbavo.so).
s_memrealtime stamps of thread 0 of every workgroup, mean over the workgroups, us since the workgroup's entry; median of 5 launches.
Thread 0 belongs to a wave that WALKS the pose chain.  The second half of the line is per wave (MBAVO_WSTAMP 0 / 1: where a wave
enters and leaves its lane-per-pixel rounds, behind the sample-parallel remainder round), split into the chain waves (the first k,
or k - 1 for cost-only) and the waves that only wait at the prologue's barriers, also since the workgroup's entry.
Usage: python tools/pose_stamps.py [case ...]     case = workload[:cost][:k2], default c2_dense"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import mba_vo_amd as M
from mba_vo_amd import workloads as wl
import bench_core as bench
ctx = M.capi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
lib = ctx.lib
lib.mbavo_debug_fused_stamps.argtypes = [C.c_void_p, C.c_int]
lib.mbavo_debug_wave_stamps.argtypes = [C.c_void_p, C.c_int]
for case in sys.argv[1:] or ["c2_dense"]:
    parts = case.split(":")
    k, with_h = (2 if "k2" in parts else 4), "cost" not in parts
    probs = bench.build_workload(parts[0], 1, k=k)[0]
    dw = wl.DeviceWorkload(probs)
    for _ in range(30): dw.step(ctx, with_h)
    torch.cuda.synchronize()
    rows, wrows = [], []
    for rep in range(5):
        buf = np.zeros(2048 * 8, np.uint64)
        dw.step(ctx, with_h); torch.cuda.synchronize()
        assert lib.mbavo_debug_fused_stamps(buf.ctypes.data, buf.size) == 0
        st = buf.reshape(2048, 8)
        n = int((st[:, 0] > 0).sum()); st = st[:n].astype(np.int64)
        rows.append(((st[:, 1:6] - st[:, :1]) / 100.0).mean(0))
        wb = np.zeros(1024 * 16 * 4, np.uint64)
        assert lib.mbavo_debug_wave_stamps(wb.ctypes.data, wb.size) == 0
        m = min(n, 1024)
        wb = wb.reshape(1024, 16, 4).astype(np.int64)[:m]
        nw = int((wb[0, :, 0] > 0).sum())
        start, end = (wb[:, :nw, 0] - st[:m, :1]) / 100.0, (wb[:, :nw, 1] - st[:m, :1]) / 100.0
        nchain = k if with_h else k - 1
        wrows.append((start[:, :nchain].mean(), start[:, nchain:].mean(), end[:, :nchain].mean(), end[:, nchain:].mean(), end.max(1).mean()))
    r, w = np.median(np.array(rows), 0), np.median(np.array(wrows), 0)
    print(case, n, "wgs", nw, "waves; mean us since entry: descs %.2f | stage A %.2f | stage B %.2f | visible %.2f | ready %.2f" % tuple(r),
          "|| rounds start: chain waves %.2f, waiting waves %.2f | rounds end: chain %.2f, waiting %.2f, last wave %.2f" % tuple(w),
          lib.mbavo_last_kernel(ctx.handle).decode(), flush=True)
