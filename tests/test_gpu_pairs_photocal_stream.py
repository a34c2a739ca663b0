"""mbavo_pairs_set_photometric on a BUSY stream (the pattern of tests/test_gpu_pairs_stream_order.py with tests/stream_backlog.py):
set_photometric immediately followed by prepare, then a second set_photometric with another table and another vignette followed
by an update with a key list -- once with the stream idle and once behind a gate, with images, depth maps and vignettes arriving
late on the stream and the host tables and the key list overwritten the moment their call has returned.  Each intake sees its own
calibration: what the object holds after the prepare and after the update is the idle run's, bit for bit, and the idle run's is the
numpy restatement's.  The first set_photometric is preceded by another one with other tables and another vignette, back to back:
the later call holds.  set_photometric promises to wait for nothing: the backlog must still be there when each of them returns.

Shapes: B = 3, L = 1, 24 x 40, pinhole intake (the calibrated launch stands where the stream-ordered copies were)."""
import numpy as np
import pytest

import pairs_device as dv
import pairs_photocal_ref as pc
import stream_backlog as sb
from mba_vo_amd import synth

pytestmark = pytest.mark.gpu

B, L, H, W = 3, 1, 24, 40


@pytest.fixture(scope="module")
def own(mbavo):
    """(S, ctx): a context on its own non-blocking stream."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    S, ctx = sb.own_stream_context(mbavo.capi)
    yield S, ctx
    S.synchronize()
    ctx.close()


def _late_set(real, stale):
    assert real.shape == stale.shape and real.dtype == stale.dtype and not np.array_equal(real, stale)
    p = sb.pinned(real)
    return sb.device_like(p), p, sb.pinned(stale)


def _inputs(seed):
    rng = np.random.default_rng(seed)
    tex = lambda s: np.stack([synth.texture_image(H, W, seed=s + 3 * b, octaves=(8, 4, 2)) for b in range(B)])
    return dict(sharp=tex(seed), blur=tex(seed + 50), depth=rng.uniform(1.0, 3.0, (B, H, W)).astype(np.float32),
                V=rng.uniform(0.03, 1.0, (1, H, W)).astype(np.float32))


def test_each_intake_sees_its_own_calibration(mbavo, own):
    from mba_vo_amd import workloads
    S, ctx = own
    lib, capi = ctx.lib, mbavo.capi
    assert lib.mbavo_pairs_photocal_opts_size() == 32
    a, b = _inputs(1), _inputs(2)
    first = {key: _late_set(a[key], b[key]) for key in ("sharp", "depth", "blur", "V")}
    first["blurV"] = _late_set(_inputs(3)["V"], _inputs(4)["V"])  # the vignette of a call that another one follows at once
    nxt = dict(blur=_late_set(b["blur"], a["blur"]), sharp=_late_set(b["sharp"][:1], a["sharp"][:1]), depth=_late_set(b["depth"][:1], a["depth"][:1]),
               V=_late_set(b["V"], a["V"]))
    G = (pc.gamma_G(2.2), pc.gamma_G(1.6))
    keys = (np.array([1], np.int32), np.array([2], np.int32))
    o = capi.PairsPhotocalOpts()
    o.scale = 0.5
    pb = workloads.PairBatch(ctx, B, L=L, H=H, W=W, S=3, k=2, N=2, border=2, cell=4, thresh=1.0)
    ok = lambda rc: rc == 0 or pytest.fail("return code %d" % rc)
    try:
        def seq(run):
            import ctypes as C
            run.place(list(first.values()))
            # (two calls back to back: neither waits, the later tables and vignette hold)
            g0, over0 = run.host(G[1], G[0])
            run.call("set_photometric 0", lambda: ok(lib.mbavo_pairs_set_photometric(pb.handle, 1, g0.ctypes.data_as(capi.c_dp), first["blurV"][0].data_ptr(),
                                                                                   C.byref(o))), after=over0, asserted=True)
            g1, over1 = run.host(G[0], G[1])
            run.call("set_photometric 1", lambda: ok(lib.mbavo_pairs_set_photometric(pb.handle, 1, g1.ctypes.data_as(capi.c_dp), first["V"][0].data_ptr(),
                                                                                   C.byref(o))), after=over1, asserted=True)
            counts = np.zeros((B, L), np.int32)
            run.call("prepare", lambda: ok(lib.mbavo_pairs_prepare(pb.handle, first["sharp"][0].data_ptr(), first["depth"][0].data_ptr(),
                                                                  first["blur"][0].data_ptr(), capi.ip(counts))))
            after_prepare = dv.read_batch(pb, counts)
            run.place(list(nxt.values()))  # (prepare reads its counts back: the second pair of calls gets a backlog and late inputs of its own)
            g2, over2 = run.host(G[1], G[0])
            run.call("set_photometric 2", lambda: ok(lib.mbavo_pairs_set_photometric(pb.handle, 1, g2.ctypes.data_as(capi.c_dp), nxt["V"][0].data_ptr(),
                                                                                   C.byref(o))), after=over2, asserted=True)
            kl, over_k = run.host(*keys)
            run.call("update", lambda: ok(lib.mbavo_pairs_update(pb.handle, nxt["blur"][0].data_ptr(), 1, capi.ip(kl), nxt["sharp"][0].data_ptr(),
                                                                nxt["depth"][0].data_ptr(), capi.ip(counts))), after=over_k)
            run.finish()
            got = dv.read_batch(pb, counts)
            return dict(prepared_ref=b"".join(g["ref"].tobytes() for g in after_prepare), prepared_cur=b"".join(g["cur"].tobytes() for g in after_prepare),
                        ref=b"".join(g["ref"].tobytes() for g in got), cur=b"".join(g["cur"].tobytes() for g in got))

        real = sb.run_case("set_photometric, prepare, set_photometric, update", S, seq)
        # the idle run on the real set is the restatement: table 1 and vignette 1 for the prepare, table 2 and vignette 2 for the update
        lut1, lut2 = pc.table(G[0], 0.5), pc.table(G[1], 0.5)
        inv1, inv2 = pc.inverse_vignette(a["V"][0]), pc.inverse_vignette(b["V"][0])
        take = lambda imgs, lut, inv: b"".join(pc.pinhole(im, lut, inv).tobytes() for im in imgs)
        assert real["prepared_ref"] == take(a["sharp"], lut1, inv1) and real["prepared_cur"] == take(a["blur"], lut1, inv1)
        ref = [pc.pinhole(a["sharp"][0], lut1, inv1), pc.pinhole(b["sharp"][0], lut2, inv2), pc.pinhole(a["sharp"][2], lut1, inv1)]
        assert real["ref"] == b"".join(r.tobytes() for r in ref) and real["cur"] == take(b["blur"], lut2, inv2)
    finally:
        pb.close()
