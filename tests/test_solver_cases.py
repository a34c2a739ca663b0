"""The cases, references and bounds of tests/solver_cases.py, checked without a device: the families have the properties they
claim, and two implementations that are NOT the code under test -- LAPACK and a plain numpy restatement of the unpivoted
LDL^T -- stay inside the very bounds tests/test_gpu_solvers.py applies to the device.  Prints the coverage table and the CPU
maxima the constants come from (profiles/r08_solver_accuracy.txt)."""
import collections
import os
import re

import numpy as np

import solver_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


def test_file_format_round_trip(tmp_path):
    runs = C.all_runs()[:7]
    C.write_cases(str(tmp_path / "c.bin"), runs)
    w = np.fromfile(str(tmp_path / "c.bin"), dtype="<i8")
    assert w[0] == C.MAGIC and w[1] == 7 and w[2] == runs[0].system.n and w[3] == C.FORMS[runs[0].form]
    n = runs[0].system.n
    assert w[4:6].view("<f8").tolist() == [runs[0].max_ratio, runs[0].max_ratio_refined]
    assert np.array_equal(w[6:6 + n * n].view("<f8").reshape(n, n).T, runs[0].system.A)
    out = [np.array([C.MAGIC, 7, 0, -1], dtype="<i8")]
    for r in runs:
        out += [np.array([r.system.n, 1, 261, 0], dtype="<i8"), r.system.b.view("<i8")]
    np.concatenate(out).tofile(str(tmp_path / "r.bin"))
    res, head = C.read_results(str(tmp_path / "r.bin"), runs)
    assert head == dict(done=7, error=0, error_case=-1) and all(np.array_equal(o["x"], r.system.b) and o["info"] == 261 for o, r in zip(res, runs))


def test_family_properties():
    S = C.all_systems()
    for s in S["dense"]:
        ref = C.reference(s)
        assert ref["pos"] and np.array_equal(s.A, s.A.T), s.name
        if s.meta["decade"] is not None:  # the pivot ratio of the STORED matrix (mpmath) sits in its decade
            lo, hi = C.DECADES[s.meta["decade"]]
            assert lo < ref["ratio"] <= hi, (s.name, ref["ratio"])
        if s.family == "well":
            assert ref["ratio"] < 1e3 and ref["kappa"] < 1e5, s.name
        if s.family == "graded":  # artificially ill conditioned: the scaling takes it away
            assert ref["kappa_s"] < 1e5 < ref["kappa"] or s.meta["decade"] == 0, (s.name, ref["kappa_s"])
        if s.family in ("neardep", "spectrum") and s.meta["decade"] > 0:  # genuinely ill conditioned: it does not
            assert ref["kappa_s"] > 1e6, (s.name, ref["kappa_s"])
    assert set(C.UNPOPULATED) <= {"spectrum_d3_n%d" % n for n in C.STANDIN_SIZES}  # (recorded in the profile file)
    for s in S["rankdef"]:
        J, x0 = s.meta["J"], s.meta["x0"]
        # exact in doubles: integers far below 2^53, and numpy's float products / sums of them are exact
        assert np.array_equal(J, np.round(J)) and np.abs(s.A).max() < 2 ** 20 and np.abs(s.b).max() < 2 ** 30
        Ji, xi = J.astype(np.int64), x0.astype(np.int64)
        assert np.array_equal(s.A, (Ji.T @ Ji).astype(float)) and np.array_equal(s.b, (Ji.T @ Ji @ xi).astype(float))
        ref = C.reference(s)
        # the minimum-norm solution: solves the system, and lies in the row space of J
        assert np.abs(s.A @ ref["x"] - s.b).max() <= 1e-9 * np.abs(s.b).max()
        P = np.linalg.pinv(J) @ J
        assert np.abs(P @ ref["x"] - ref["x"]).max() <= 1e-10 * np.abs(ref["x"]).max()
        if "untouched" in s.meta:
            assert not np.any(ref["x"][s.meta["untouched"]]) and not np.any(s.A[s.meta["untouched"]])
    for s in S["threshold"]:
        n = s.n
        ref = C.reference(s)
        lam = np.abs(s.meta["lam"]) if s.kind == "spectral" else np.abs(ref["lam"])
        thr = n * C.EPS * lam.max()
        assert all(v >= 100 * thr or v <= thr / 100 for v in lam), s.name
        if s.kind == "spectral":  # the exact construction against LAPACK on the stored matrix
            ev = np.sort(np.abs(np.linalg.eigvalsh(s.A)))[::-1]
            assert np.abs(ev - np.sort(lam)[::-1]).max() <= 50 * n * C.EPS * lam.max()
    for s in S["gate"]:
        if "exact_ratio" in s.meta and s.kind == "spd":  # the exactly known pivots are what mpmath finds
            ref = C.reference(s)
            assert ref["ratio"] == s.meta["exact_ratio"], (s.name, ref["ratio"])
            L, d = C.ldlt_unpivoted(s.A)
            assert np.array_equal(np.sort(d), np.sort(ref["pivots"])), s.name  # ... and what float64 computes: every step exact
        if s.meta.get("side") == "refuse" and np.all(np.isfinite(s.A)):
            assert not C.reference(s)["pivots"][-1] > 0, s.name


def _cpu_solutions(s, ref):
    """name -> x for the implementations that apply to the system."""
    out = {}
    n = s.n
    if s.kind in ("spd", "general"):
        out["lapack solve"] = np.linalg.solve(s.A, s.b)
    if s.kind == "spd":
        import scipy.linalg as sl
        out["lapack potrs"] = sl.cho_solve(sl.cho_factor(s.A), s.b)
        L, d = C.ldlt_unpivoted(s.A)
        out["numpy LDL^T"] = C.ldlt_apply(L, d, s.b)
    out["lapack pinv"] = np.linalg.pinv(s.A, rcond=n * C.EPS, hermitian=True) @ s.b
    return out


def test_cpu_implementations_stay_inside_the_bounds():
    S = C.all_systems()
    scaled, kappa = collections.defaultdict(float), collections.defaultdict(float)
    worst = {}
    standin = [s for s in S["dense"] + S["gate"] + S["extra"] if s.kind == "spd" and s.family != "scaled"]
    for s in standin:
        ref = C.reference(s)
        if ref["ratio"] > C.FAST_RATIO or not np.any(s.b):
            continue  # the scaled bound is applied to what the plain stand-in accepts
        for name, x in _cpu_solutions(s, ref).items():
            if name != "lapack pinv":
                q = C.scaled_error_ratio(s, ref, x)
                scaled[(name, s.family)] = max(scaled[(name, s.family)], q)
                worst[("scaled", name)] = max(worst.get(("scaled", name), (0, "")), (q, s.name))
    jac = {id(r.system): r.system for r in C.all_runs() if r.form not in C.STANDINS and r.system.family != "scaled"}
    for s in jac.values():
        ref = C.system_reference(s)
        for name, x in _cpu_solutions(s, ref).items():
            q = C.kappa_error_ratio(s, ref, x)
            kappa[(name, s.family)] = max(kappa[(name, s.family)], q)
            worst[("kappa", name)] = max(worst.get(("kappa", name), (0, "")), (q, s.name))
            if s.kind == "spd" and name != "lapack pinv":  # eig / ldlt are held to the scaled bound on these as well
                q = C.scaled_error_ratio(s, ref, x)
                scaled[(name, s.family)] = max(scaled[(name, s.family)], q)
                worst[("scaled", name)] = max(worst.get(("scaled", name), (0, "")), (q, s.name))
    print("\nCPU maxima, scaled error / (n eps kappa_s |x|):")
    for k in sorted(scaled):
        print("  %-14s %-10s %.3e" % (k + (scaled[k],)))
    print("CPU maxima, error / (n eps kappa |x|):")
    for k in sorted(kappa):
        print("  %-14s %-10s %.3e" % (k + (kappa[k],)))
    print("worst:", worst)
    ms, mk = max(scaled.values()), max(kappa.values())
    print("maximum scaled %.3e -> C_SCALED = 8 x = %.3g (in use: %.3g); maximum kappa %.3e -> C_KAPPA = 8 x = %.3g (in use: %.3g)"
          % (ms, 8 * ms, C.C_SCALED, mk, 8 * mk, C.C_KAPPA))
    assert ms <= C.C_SCALED and mk <= C.C_KAPPA
    # the constants are 8x the maxima measured when they were set; another LAPACK build may round differently, not 8x differently
    assert C.C_SCALED / 8 <= 4 * ms and C.C_KAPPA / 8 <= 4 * mk


def test_refined_reference_rule_meets_the_refined_bar():
    """Where the restated rule (exact residuals) accepts, its own x is within 1e-12 |x| of the reference: the bar is reachable."""
    for s in C.all_systems()["dense"]:
        ref = C.reference(s)
        if C.must_accept_refined(s, ref):
            ok, steps, x = C.refine_rule(s.A, s.b, 0.0, C.REFINED_RATIO)
            assert ok and steps == ref["refine_steps"] <= C.REFINE_STEPS
            assert np.abs(x - ref["x"]).max() <= C.REFINED_TOL * np.abs(ref["x"]).max(), s.name


def test_coverage_conditions():
    S = C.all_systems()
    runs = C.all_runs()
    dense = S["dense"]
    # 1. the must-accept set: at least one case per stand-in size in each of (1e8, 1e10] and (1e10, 1e12]
    must = collections.Counter()
    for s in dense:
        ref = C.reference(s)
        if C.must_accept_refined(s, ref):
            must[(s.n, C.decade_of(ref["ratio"]))] += 1
    for n in C.STANDIN_SIZES:
        assert must[(n, 1)] >= 1 and must[(n, 2)] >= 1, (n, must)
    # 2. cases left out for sitting next to a gate: at most 5 % of the dense cases
    out = sum(1 for s in dense for g in (C.FAST_RATIO, C.REFINED_RATIO) if abs(C.reference(s)["ratio"] / g - 1) <= C.GATE_MARGIN)
    assert out <= 0.05 * len(dense), out
    # 3. every form at every size lm_batch.hip dispatches it at: the register form at 12 / 18 / 24, the workgroup form at every even
    # 6 N from 30 to 60 in both of its widths, eig_solve up to kEigMaxN, the one-wave SVD and the pivoted LDL^T up to 96
    sizes = collections.defaultdict(set)
    for r in runs:
        sizes[r.form].add(r.system.n)
    six = lambda lo, hi: set(range(lo, hi + 1, 6))
    assert sizes["regs"] == six(12, 24) and sizes["coop64"] == six(30, 60) == sizes["coop256"]
    assert sizes["eig"] == six(12, C.EIG_MAX_N) and sizes["svd"] == six(12, 96) and sizes["ldlt"] == six(12, 96)
    # all three lanes-per-pair choices of svd_sweeps: 4 (n <= 32, N6 >= 4), 2 (n <= 64), 1
    assert {24, 30} <= sizes["svd"] and {36, 60} <= sizes["svd"] and {12, 18, 66, 96} <= sizes["svd"]
    table = collections.Counter()
    for r in runs:
        ratio = C.system_reference(r.system)["ratio"] if r.system.kind in ("spd", "embedded") else None
        dec = "-" if ratio is None or not np.isfinite(ratio) else "<=1e2" if ratio <= 1e2 else ">1e13" if ratio > 1e13 else "d%d" % C.decade_of(ratio)
        table[(r.form, r.system.n, dec)] += 1
    cols = ["<=1e2", "d0", "d1", "d2", "d3", ">1e13", "-"]
    print("\ncases per form, size and pivot-ratio decade (d0 = (1e2, 1e8], d1 = (1e8, 1e10], d2 = (1e10, 1e12], d3 = (1e12, 1e13); - = not positive definite)")
    print("%-8s %4s " % ("form", "n") + " ".join("%6s" % c for c in cols))
    for form in C.FORMS:
        for n in sorted(sizes[form]):
            print("%-8s %4d " % (form, n) + " ".join("%6d" % table[(form, n, c)] for c in cols))
    print("runs %d, systems %d; must-accept systems %d (per size and decade: %s); left out next to a gate %d of %d dense (%.1f %%)"
          % (len(runs), sum(len(v) for v in S.values()), sum(must.values()), dict(sorted(must.items())), out, len(dense), 100.0 * out / len(dense)))
    print("unpopulated:", C.UNPOPULATED)


def test_default_mode_of_the_check_uses_the_same_constant():
    src = open(os.path.join(HERE, "harness", "solver_check.hip")).read()
    m = re.search(r"kScaledBoundC\s*=\s*([0-9.eE+-]+)", src)
    assert m and float(m.group(1)) == C.C_SCALED
