"""mbavo_pairs_prune_keypoints without a GPU: the entries exist in the library, the header and the binding, the structs have the
sizes the header states, NULL handles are rejected -- and the specification, restated in numpy (tests/pairs_prune_ref.py), is held
to hand-made arrays: the survivors keep their order, the tail keeps its bits, the criteria are counted in their fixed order, a flag
byte of 32 or more never drops, min_keep acts exactly at min_keep.  Every test asks the library for the calls first: none passes
where they do not exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pairs_prune_ref as pref

E_ARG = -1
NEW = ["mbavo_pairs_prune_opts_size", "mbavo_pairs_prune_size", "mbavo_pairs_prune_keypoints", "mbavo_pairs_prune_stats"]


@pytest.fixture(autouse=True)
def the_calls_exist(mbavo):
    """The restatement restates a call of the library: its record is the binding's."""
    lib = mbavo.load()
    assert lib.mbavo_pairs_prune_size() == C.sizeof(mbavo.capi.PairsPrune)
    assert lib.mbavo_pairs_prune_opts_size() == C.sizeof(mbavo.capi.PairsPruneOpts)


def test_entries_and_struct_sizes(mbavo):
    lib, capi = mbavo.load(), mbavo.capi
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mbavo.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS and name in header
    assert lib.mbavo_pairs_prune_opts_size() == C.sizeof(capi.PairsPruneOpts) == 16 + 8 + 8 + 16 + 8 + 16
    assert lib.mbavo_pairs_prune_size() == C.sizeof(capi.PairsPrune) == 32
    assert "typedef struct mbavo_pairs_prune_opts {    /* zero-initialise; 72 bytes, no padding */" in header
    assert "struct mbavo_pairs_prune {                 /* one per (listed pair, reported level); 32 bytes, no padding */" in header
    assert "#define MBAVO_ABI_VERSION 3" in header and lib.mbavo_abi_version() == 3
    # the fields in the header's order
    assert [f[0] for f in capi.PairsPruneOpts._fields_] == ["level", "apply", "drop_mask", "use_filter", "min_info", "min_obs", "rej_limit", "z_min", "z_max",
                                                            "check_depth", "min_keep", "reserved"]
    assert [f[0] for f in capi.PairsPrune._fields_] == ["status", "num_before", "num_kept", "by_flag", "by_depth", "by_filter", "skipped", "pad"]
    assert capi.PairsPruneOpts.drop_mask.offset == 8 and capi.PairsPruneOpts.min_info.offset == 16 and capi.PairsPruneOpts.z_min.offset == 32
    assert capi.PairsPruneOpts.min_keep.offset == 52


def test_null_handles_are_rejected(mbavo):
    """(each bad argument of a live object: tests/test_gpu_pairs_prune.py, an object needs a device)"""
    lib, capi = mbavo.load(), mbavo.capi
    assert pref.call(lib, None, None, pref.opts_struct(capi), out=(capi.PairsPrune * 4)()) == E_ARG
    assert pref.call(lib, None, [0], pref.opts_struct(capi, apply=1)) == E_ARG
    assert lib.mbavo_pairs_prune_stats(None, (C.c_longlong * 3)()) == E_ARG


def test_binding_methods_exist(mbavo):
    from mba_vo_amd import workloads
    assert all(callable(getattr(workloads.PairBatch, n)) for n in ("prune_keypoints", "prune_stats"))


def _arrays(cap, seed=0):
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 64, (cap, 2)).astype(np.float64)
    z = rng.uniform(1.0, 5.0, cap)
    state = dict(mu=rng.uniform(0.2, 1.0, cap), info=rng.uniform(1.0, 9.0, cap), n_obs=rng.integers(0, 9, cap).astype(np.int32),
                 n_rej=rng.integers(0, 4, cap).astype(np.int32))
    return xy, z, state


def test_order_is_kept_and_the_tail_is_untouched(mbavo):
    cap, K = 12, 9
    xy, z, st = _arrays(cap)
    flags = np.array([0, 3, 0, 0, 3, 3, 0, 3, 0, 3, 3, 3], np.uint8)  # (the bytes from K on are not read)
    r = pref.prune(K, xy, z, st, flags=flags, drop_mask=1 << 3)
    src = [0, 2, 3, 6, 8]
    assert r["K"] == 5 and r["keep"].tolist() == [1, 0, 1, 1, 0, 0, 1, 0, 1]
    assert np.array_equal(r["xy"][:5], xy[src]) and np.array_equal(r["z"][:5], z[src])
    for key in st:
        assert np.array_equal(r["state"][key][:5], st[key][src]) and np.array_equal(r["state"][key][5:], st[key][5:]), key
    # from the new count on: the bits the arrays held, the dropped and the moved ones' old copies included
    assert np.array_equal(r["xy"][5:], xy[5:]) and np.array_equal(r["z"][5:], z[5:])
    assert r["record"] == (0, 9, 5, 4, 0, 0, 0, 0)
    # apply = 0: the same record and keep bytes, nothing moved
    d = pref.prune(K, xy, z, st, flags=flags, drop_mask=1 << 3, apply=0)
    assert d["record"] == r["record"] and np.array_equal(d["keep"], r["keep"]) and d["K"] == K
    assert np.array_equal(d["xy"], xy) and np.array_equal(d["z"], z) and all(np.array_equal(d["state"][key], st[key]) for key in st)
    # without a filter state the keypoints move alone
    n = pref.prune(K, xy, z, None, flags=flags, drop_mask=1 << 3)
    assert n["state"] is None and np.array_equal(n["z"], r["z"])


def test_every_drop_is_counted_under_the_first_criterion(mbavo):
    K = 6
    xy, z, st = _arrays(K)
    flags = np.array([1, 0, 0, 0, 1, 0], np.uint8)
    z[:] = [2.0, np.nan, 2.0, 2.0, 0.0, 2.0]             # 0: flag; 1: depth; 4: flag AND depth AND filter -> flag
    st["n_rej"][:] = [0, 5, 5, 0, 5, 0]                   # 1: depth AND filter -> depth; 2: filter alone
    st["info"][:] = 4.0
    st["n_obs"][:] = 3
    r = pref.prune(K, xy, z, st, flags=flags, drop_mask=1 << 1, check_depth=1, use_filter=1, rej_limit=5)
    assert r["verdicts"].tolist() == [pref.BY_FLAG, pref.BY_DEPTH, pref.BY_FILTER, pref.KEEP, pref.BY_FLAG, pref.KEEP]
    assert r["record"] == (0, 6, 2, 2, 1, 1, 0, 0) and r["K"] == 2
    # each filter criterion, and zero meaning "not asked"
    st["info"][:] = [0.5, 1.0, 4.0, np.nan, 4.0, 4.0]
    st["n_obs"][:] = [3, 3, 1, 3, 2, 3]
    st["n_rej"][:] = 0
    z[:] = 2.0
    r = pref.prune(K, xy, z, st, use_filter=1, min_info=1.0, min_obs=2)
    assert r["verdicts"].tolist() == [3, 0, 3, 0, 0, 0]   # info < 1.0; n_obs < 2; the NaN info and the limits themselves stay
    assert pref.prune(K, xy, z, st, use_filter=1)["record"] == (0, 6, 6, 0, 0, 0, 0, 0)
    assert pref.prune(K, xy, z, st, use_filter=0, min_info=1.0, min_obs=2)["K"] == 6
    # a zeroed options struct drops nothing, whatever the flags say
    assert pref.prune(K, xy, z, st, flags=flags)["K"] == 6


def test_depth_limits_are_inclusive(mbavo):
    z = np.array([np.nan, 0.0, 0.5, np.nextafter(0.5, 0.0), 8.0, np.nextafter(8.0, 9.0), np.inf, -1.0, 1e-2, 0.009])
    xy = np.zeros((len(z), 2))
    r = pref.prune(len(z), xy, z, check_depth=1, z_min=0.5, z_max=8.0)
    assert r["keep"].tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 0, 0] and r["record"][4] == 8
    r = pref.prune(len(z), xy, z, check_depth=1)  # z_min 0: 1e-2, z_max 0: no upper limit -- +inf is not finite
    assert r["keep"].tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 1, 0]
    assert pref.prune(len(z), xy, z, z_min=0.5, z_max=8.0)["K"] == len(z)  # check_depth = 0


def test_a_flag_of_32_or_more_never_drops(mbavo):
    flags = np.array([0, 31, 32, 33, 63, 64, 255, 1], np.uint8)
    xy, z, _ = _arrays(8)
    r = pref.prune(8, xy, z, flags=flags, drop_mask=0xFFFFFFFF)
    assert r["keep"].tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    r = pref.prune(8, xy, z, flags=flags, drop_mask=(1 << 31) | 1)  # bit f of the mask, not f mod 32
    assert r["keep"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]


def test_min_keep_acts_exactly_at_min_keep(mbavo):
    K = 10
    xy, z, st = _arrays(K)
    flags = np.zeros(K, np.uint8)
    flags[[1, 4, 7]] = 2  # 7 survivors
    at = pref.prune(K, xy, z, st, flags=flags, drop_mask=1 << 2, min_keep=7)
    assert at["K"] == 7 and at["record"] == (0, 10, 7, 3, 0, 0, 0, 0)
    short = pref.prune(K, xy, z, st, flags=flags, drop_mask=1 << 2, min_keep=8)
    assert short["K"] == K and short["record"] == (0, 10, 10, 3, 0, 0, 1, 0) and short["keep"].tolist() == [1] * K
    assert np.array_equal(short["xy"], xy) and np.array_equal(short["z"], z) and all(np.array_equal(short["state"][key], st[key]) for key in st)
    # a level that loses nothing is not "held back", however few keypoints it has
    assert pref.prune(K, xy, z, st, min_keep=50)["record"] == (0, 10, 10, 0, 0, 0, 0, 0)
    assert pref.prune(0, xy[:0], z[:0], None, min_keep=5)["record"] == (0, 0, 0, 0, 0, 0, 0, 0)
