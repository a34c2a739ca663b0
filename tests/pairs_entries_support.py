"""What the tests of the option-laden objects A - D share on the entries a pairs object hands to the engine (helper, no test in
it): every entry held bit for bit to pairs_oracle.host_levels (tests/test_gpu_pairs_oracle.py; under a calibrated intake
tests/test_gpu_pairs_photocal_options.py), and one mbavo_eval_batch of entries held to the oracle on the rebuilt problems, with the
bounds of tests/test_gpu_pairs_oracle.py's docstring."""
import types

import numpy as np

import eval_support as es
import pairs_oracle as po
import pairs_report_ref as rr
import pairs_track_support as tsup


def same_arrays(got, want, tag):
    for key in ("ref", "grad", "xy", "z", "pattern", "cap", "exp", "kt", "kR", "start", "intr"):
        assert np.array_equal(got[key], want[key]), (tag, key)
    assert np.array_equal(got["curs"][0], want["curs"][0]), (tag, "cur")
    assert all(got[key] == want[key] for key in ("S", "F", "K", "P", "N", "H", "W", "fmt", "t0", "dt", "huber")), tag


def check_entries(orc, capi, pb, name, c=None, intake=None):
    """Every (pair, level) entry of the object against pairs_oracle.host_levels(name, c, intake); returns the rebuilt problems."""
    o = po.OBJECTS[name]
    want = po.host_levels(name, c, intake)
    got = tsup.rebuilt(orc, capi, pb, o["k"])
    for b in range(o["B"]):
        for l in range(o["L"]):
            q, e = pb.array[b * o["L"] + l], got[b][l][1][-1]
            tag = (name, b, l)
            assert (q.H, q.W, q.S, q.P, q.N, q.F, q.grad_fp16) == (o["H"] >> l, o["W"] >> l, o["S"], o["P"], o["N"], 1, o["fmt"]), tag
            assert q.K == want[b][l]["K"] > 0 and not q.d_outlier and q.num_bad == 0, tag
            assert list(q.intrinsics) == [v / float(1 << l) for v in po.to_intr(o, b)], tag  # the pair's camera's, exactly
            assert q.h_start_idx[0] == o["start"] and q.huber_a == po.HUBER, tag
            if o["fmt"] == 2:
                assert np.array_equal(e["word_I"], e["ref"]), tag  # the word's intensity is the u8 image's
            same_arrays(e, want[b][l], tag)  # the restatements the CPU file's conditions were asserted on
    return got


def eval_batch(mbavo, ctx, arr, n, k, with_hessian):
    import torch
    capi = mbavo.capi
    E = rr.packed_len(k)
    Ks = [arr[e].K for e in range(n)]
    fb = torch.zeros(n * E, dtype=torch.float64, device="cuda:0")
    pc = torch.zeros(max(sum(Ks), 1), dtype=torch.float64, device="cuda:0")
    valid = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    capi.check(ctx.lib.mbavo_eval_batch(ctx.handle, n, arr, k, 1 if with_hessian else 0, fb.data_ptr(), pc.data_ptr(), valid.data_ptr()), "mbavo_eval_batch")
    torch.cuda.synchronize()
    off = np.concatenate([[0], np.cumsum(Ks)])
    pcs = pc.cpu().numpy()
    return fb.cpu().numpy().reshape(n, E), [pcs[off[e]:off[e + 1]] for e in range(n)], valid.cpu().numpy()


def check_evaluation(orc, mbavo, ctx, arr, flat, k, tag):
    """The device's blocks, patch costs and valid counts of the entries `arr` against orc.evaluate of the rebuilt problems `flat`."""
    n = len(flat)
    fb, pcs, valid = eval_batch(mbavo, ctx, arr, n, k, True)
    fc, _, vc = eval_batch(mbavo, ctx, arr, n, k, False)
    worst = dict(block=0.0, patch=0.0, cost_only=0.0, flipped=0)
    for e, (p, keep) in enumerate(flat):
        ro = orc.evaluate(p)
        want = ro["frame_blocks"][0]
        tol = es.tol(types.SimpleNamespace(K=p.K, F=p.F, P=p.P))
        rel = float(np.abs(fb[e] - want).max() / max(np.abs(want).max(), 1e-300))
        worst["block"] = max(worst["block"], rel / tol)
        assert rel < tol, (tag, e, rel, tol)
        assert valid[e] == orc.count_valid(p)[0] == vc[e] and valid[e] > 6, (tag, e, valid[e])
        want_pc = ro["patch_blocks"][0][:, 0]
        mism = pcs[e] != want_pc
        worst["flipped"] = max(worst["flipped"], int(mism.sum()))
        assert mism.sum() <= max(2, int(0.01 * want_pc.size)), (tag, e, int(mism.sum()), want_pc.size)
        d = float(np.abs(pcs[e] - want_pc).max() / max(np.abs(want_pc).max(), 1e-300))
        worst["patch"] = max(worst["patch"], d / 1e-5)
        assert d <= 1e-5, (tag, e, d)
        c = abs(fc[e, 0] - fb[e, 0]) / max(abs(fb[e, 0]), 1e-300)
        worst["cost_only"] = max(worst["cost_only"], c / 1e-11)
        assert c <= 1e-11, (tag, e, c)
    print("evaluation %s: blocks %.2e of es.tol, patch costs %.2e of 1e-5 (at most %d of an entry differ at all), cost-only %.2e of 1e-11"
          % (tag, worst["block"], worst["patch"], worst["flipped"], worst["cost_only"]))
