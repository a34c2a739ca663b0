"""What tests/test_gpu_pairs_oracle.py rests on, asserted without a GPU: the gradient-format decodes of tests/pairs_oracle.py, and for
each of its four objects -- built here from the numpy restatements that are byte-exact to the device -- that every entry has
keypoints, every level-0 entry more than 6 valid pixels and a K that is no multiple of 64, the every-candidate object a level-0 K
beyond 4096; and that the comparison of the LM loops cannot flip on a rounding: the oracle and its contracted build
(orc.fma_variant()) give the same (level, iteration, kind, outlier count) sequence for every pair, no patch cost lies within 1e-6
relative of its chi bound in any detection, and at most one pair of the whole table ends with an information matrix that is
singular to working precision (cond > 1e12).  The spread of the two builds (costs along the trace, final knots) is printed: it is
the yardstick profiles/r25_pairs_oracle.txt lists beside the device's figures."""
import numpy as np
import pytest

import pairs_oracle as po
import pairs_report_ref as rr
from mba_vo_amd import synth

NAMES = sorted(po.OBJECTS)
_RUNS = {}


def test_half_decode_on_hand_made_words_and_an_image():
    words = np.array([0x0000, 0x8000, 0x3800, 0xb800, 0x57f8, 0xd7f8, 0x3c00, 0x4000], np.uint16)  # 0, -0, .5, -.5, 127.5, -127.5, 1, 2
    got = po.decode_half(words, 1, 4)
    assert got.dtype == np.float32 and got.ravel().tolist() == [0.0, -0.0, 0.5, -0.5, 127.5, -127.5, 1.0, 2.0]
    assert np.signbit(got[0, 0, 1])
    img = synth.texture_image(37, 53, seed=4, octaves=(8, 4))
    img[5, 4:9] = [0, 7, 255, 9, 0]
    g = synth.image_gradients(img)
    back = po.decode_half(po.encode_half(g), 37, 53)
    assert np.array_equal(back.view(np.uint32), g.view(np.uint32))  # central differences of an 8-bit image are whole halves: lossless
    odd = np.array([[[0.1, 1000.3]]], np.float32)                    # what is not: the half-rounded value
    assert np.array_equal(po.decode_half(po.encode_half(odd), 1, 1), odd.astype(np.float16).astype(np.float32))


def test_packed_decode_on_hand_made_words_and_an_image():
    word = lambda I, kx, ky: I | ((kx & 0x1ff) << 8) | ((ky & 0x1ff) << 23)
    cases = [(0, 0, 0), (255, 255, -255), (17, -255, 255), (200, 1, -1), (3, -1, 1), (128, 254, -254)]
    I, g = po.decode_packed(np.array([word(*c) for c in cases], np.uint32), 2, 3)
    assert I.ravel().tolist() == [c[0] for c in cases]
    assert g.reshape(-1, 2).tolist() == [[0.5 * c[1], 0.5 * c[2]] for c in cases]
    # bits 17-22 belong to nothing: they change nothing
    I2, g2 = po.decode_packed(np.array([word(*c) | (0x3f << 17) for c in cases], np.uint32), 2, 3)
    assert np.array_equal(I2, I) and np.array_equal(g2, g)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    img[5, 4:9] = [0, 7, 255, 9, 0]
    img[10:15, 20] = [0, 7, 255, 9, 0]
    I, g = po.decode_packed(synth.pack_keyframe(img), 37, 53)
    want = synth.image_gradients(img)
    assert np.array_equal(I, img) and np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert g.min() == -127.5 and g.max() == 127.5


def _run(orc, name):
    """Both builds' LM loops on every pair of an object (made once): dict(levels, oracle [per pair], fma [per pair] or None)."""
    if name not in _RUNS:
        levels = po.host_levels(name)
        fma = orc.fma_variant()
        runs = {}
        for tag, lib in (("oracle", orc), ("fma", fma)):
            runs[tag] = None if lib is None else [po.oracle_lm_levels(lib, [po.problem_of(lib, dict(e)) for e in pair]) for pair in levels]
        _RUNS[name] = dict(levels=levels, **runs)
    return _RUNS[name]


@pytest.mark.parametrize("name", NAMES)
def test_the_objects_are_what_the_gpu_tests_rest_on(orc, name):
    o = po.OBJECTS[name]
    levels = po.host_levels(name)
    assert len(levels) == o["B"] and o["B"] in (3, 4) and o["L"] in (2, 3)
    Ks = np.array([[e["K"] for e in pair] for pair in levels])
    print("object %s: K per (pair, level) %s" % (name, Ks.tolist()))
    assert (Ks > 0).all()
    assert (Ks[:, 0] % 64 != 0).all()
    if name == "C":
        assert (Ks[:, 0] > 4096).all()
    if name == "D":
        assert (Ks[:, 0] < 64).any() and len(set(Ks[:, 0].tolist())) == o["B"]
    for b, pair in enumerate(levels):
        p, keep = po.problem_of(orc, dict(pair[0]))
        assert orc.count_valid(p)[0] > 6, (name, b)
        assert pair[0]["start"][0] == o["start"] and all(e["start"][0] == o["start"] for e in pair)
        for l, e in enumerate(pair):
            assert (e["H"], e["W"]) == (o["H"] >> l, o["W"] >> l) and e["intr"].tolist() == [v / (1 << l) for v in po.to_intr(o, b)]
    if o["cam_of"] is not None:  # the cameras of a set differ in every intrinsic: a pair given its neighbour's shows
        K4 = [cam["to_intr"] for cam in o["cams"]]
        assert all(K4[i][g] != K4[j][g] for i in range(len(K4)) for j in range(i) for g in range(4))
    if name == "B":
        again = po.host_levels(name, po.second_frame(name))
        K2 = np.array([[e["K"] for e in pair] for pair in again])
        assert (K2 > 0).all() and (K2[:, 0] % 64 != 0).all() and not np.array_equal(K2[2], Ks[2]) and np.array_equal(K2[[0, 1, 3]], Ks[[0, 1, 3]])


@pytest.mark.parametrize("name", NAMES)
def test_the_lm_comparison_cannot_flip_on_a_rounding(orc, name):
    r = _run(orc, name)
    if r["fma"] is None:
        pytest.skip("the host compiler or CPU has no FMA: no contracted build to compare with")
    worst_cost = worst_knot = 0.0
    for b, (a, f) in enumerate(zip(r["oracle"], r["fma"])):
        assert [t[:4] for t in a["trace"]] == [t[:4] for t in f["trace"]], (name, b)
        assert a["margin"] > 1e-6 and f["margin"] > 1e-6, (name, b, a["margin"], f["margin"])
        for x, y in zip(a["trace"], f["trace"]):
            worst_cost = max(worst_cost, max(abs(x[i] - y[i]) / max(1.0, abs(x[i])) for i in (5, 6)))
        worst_knot = max(worst_knot, float(np.abs(a["kt"] - f["kt"]).max()), float(np.abs(a["kR"] - f["kR"]).max()))
        kinds = [t[2] for t in a["trace"]]
        print("object %s pair %d: %d records, accepted %d rejected %d invalid %d, chi margin %.2e, quality margin %.2e"
              % (name, b, len(kinds), kinds.count(1), kinds.count(2), kinds.count(3), a["margin"], a["quality_margin"]))
    assert any(t[2] == 1 for a in r["oracle"] for t in a["trace"])  # the knots move
    print("object %s: oracle against its FMA build: costs %.3e (of the 1e-6 allowed the device), knots %.3e (of 1e-5)" % (name, worst_cost, worst_knot))
    assert worst_cost < 1e-4 and worst_knot < 1e-4  # (both builds end at the same place: the seeds were chosen for it)


def _report_of(orc, name, b, run):
    """The report restatement of pair b at the oracle's final knots, from the oracle's level-0 block: (want, near)."""
    o = po.OBJECTS[name]
    e = dict(run["levels"][b][0], kt=run["oracle"][b]["kt"].ravel().copy(), kR=run["oracle"][b]["kR"].ravel().copy())
    p, keep = po.problem_of(orc, e)
    fb, pc = po.evaluate0(orc, p)
    s, k = o["start"], o["k"]
    want = rr.report(fb[0], run["oracle"][b]["kt"][s:s + k], run["oracle"][b]["kR"][s:s + k], pc[0], orc.count_valid(p)[0], e["K"], o["P"], k, 3.0)
    return want, rr.near_the_bound(pc[0], want["mu"], want["bound"], e["K"])


def test_at_most_one_pair_of_the_table_ends_singular(orc):
    singular = []
    for name in NAMES:
        run = _run(orc, name)
        for b in range(po.OBJECTS[name]["B"]):
            want, near = _report_of(orc, name, b, run)
            assert not near.any(), (name, b)
            cond = np.linalg.cond(want["info_unit"])
            print("object %s pair %d: cond(info_unit) %.3e, status %d, flagged %d of %d" % (name, b, cond, want["status"], want["num_flagged"], want["num_stat"]))
            if want["status"] != 0 or cond > 1e12:
                singular.append((name, b, cond))
    assert len(singular) <= 1, singular
