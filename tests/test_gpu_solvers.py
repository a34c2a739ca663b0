"""-m gpu: the device solvers of lm_solvers.h, case by case, against mpmath references (tests/solver_cases.py).

The cases go through tests/harness/solver_check.hip's data mode in ONE process (one launch at a time, stopping at the first
failed launch), under a time limit.  What is asserted, per case:
  * launch error 0, no NaN in an accepted result;
  * plain stand-in (gates 1e8 / 0 and 1e8 / 1e13): accepted exactly when every pivot is positive and the pivot ratio is <= 1e8
    (exact pivots for the gate cases, mpmath pivots for the dense ones, those within 1 +- 1e-6 of the gate left out), accepted
    results inside the scaled LDL^T forward bound;
  * refined stand-in: accepted results within 1e-12 |x|_inf of the reference, acceptance REQUIRED on the must-accept set,
    refusal required for a non-positive pivot, a NaN and a ratio above the gate;
  * svd / eig / ldlt: C_KAPPA n eps kappa |x| against the reference (kappa over the kept eigenvalues); the forms built on a
    Cholesky factor (eig's preconditioned path, the pivoted ldlt) also inside the scaled bound on positive definite systems;
    untouched knots exactly 0; eig's path bit (preconditioned for positive definite systems, plain for indefinite ones and for
    exactly zero pivots; a zero pivot that is a rounding residue may go either way);
  * (2^s A) x = 2^s b, s = +-200: the same bits as the unscaled system in every form.  pivot_reciprocal has no range scaling, but
    pivots of 2^+-200 x (1 ... 1e13) and their reciprocals are normal numbers: nothing is refused, nothing changes.
"""
import collections
import os
import subprocess

import numpy as np
import pytest

import solver_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "harness", "solver_check_bin")
SOURCES = (os.path.join(HERE, "harness", "solver_check.hip"), os.path.join(HERE, "..", "mba-vo_amd", "csrc", "lm_solvers.h"))


def fresh_binary():
    """solver_check_bin, rebuilt when it is missing or older than its sources (a stale one would lack the data mode)."""
    if not os.path.exists(EXE) or any(os.path.getmtime(p) > os.path.getmtime(EXE) for p in SOURCES):
        subprocess.run(["bash", os.path.join(HERE, "harness", "build.sh")], check=True)
    return EXE


@pytest.fixture(scope="module")
def results(mbavo, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = fresh_binary()
    runs = C.all_runs()
    d = tmp_path_factory.mktemp("solver_cases")
    cin, cout = str(d / "cases.bin"), str(d / "results.bin")
    C.write_cases(cin, runs)
    r = subprocess.run([exe, "--cases", cin, "--out", cout], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "SOLVER CASES RUN %d" % len(runs) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res, head = C.read_results(cout, runs)
    assert head["done"] == len(runs) and head["error"] == 0 and head["error_case"] == -1, head
    return runs, res


class Report:
    """Collects every failure (one assert at the end: a wrong solver shows all the cases it breaks) and the maxima per form and family."""

    def __init__(self):
        self.bad, self.maxima, self.counts = [], collections.defaultdict(float), collections.Counter()

    def check(self, cond, run, what):
        if not cond:
            self.bad.append("%r: %s" % (run, what))

    def figure(self, key, v):
        self.maxima[key] = max(self.maxima[key], v)

    def finish(self):
        for k in sorted(self.maxima):
            print("max %-58s %.3e" % (" ".join(str(x) for x in k), self.maxima[k]))
        for k in sorted(self.counts):
            print("count %-56s %d" % (k, self.counts[k]))
        assert not self.bad, "%d failures:\n" % len(self.bad) + "\n".join(self.bad[:60])


def test_every_launch_succeeded_and_accepted_results_are_finite(results):
    runs, res = results
    rep = Report()
    for r, o in zip(runs, res):
        rep.check(o["err"] == 0, r, "hipError_t %d" % o["err"])
        accepted = o["ok"] if r.form in C.STANDINS else np.all(np.isfinite(r.system.A))
        if accepted:
            rep.check(np.all(np.isfinite(o["x"])), r, "NaN / inf in an accepted result")
    rep.finish()


def test_plain_standin_verdict_and_forward_bound(results):
    """Gates (1e8, 0) and, where the ratio is <= 1e8, the production pair (1e8, 1e13)."""
    runs, res = results
    rep = Report()
    for r, o in zip(runs, res):
        s = r.system
        if r.form not in C.STANDINS or r.max_ratio != C.FAST_RATIO:
            continue
        ref = C.system_reference(s)
        verdict = C.expected_plain_verdict(s, ref, r.max_ratio)
        if verdict is None:
            rep.counts["left out next to the gate"] += 1
            continue
        if r.max_ratio_refined == 0:
            rep.check(o["ok"] == verdict, r, "accepted %d, required %d (pivot ratio %.17g)" % (o["ok"], verdict, s.meta.get("exact_ratio", ref["ratio"])))
        elif verdict:
            rep.check(o["ok"], r, "refused below the fast gate")
        if verdict and o["ok"]:
            rep.counts["plain accepted"] += 1
            q = C.scaled_error_ratio(s, ref, o["x"])
            rep.figure((r.form, s.family, "scaled error / (n eps kappa_s |x|)"), q)
            rep.check(q <= C.C_SCALED, r, "scaled error ratio %.3e > %.3g" % (q, C.C_SCALED))
            if "bitwise" in s.meta:  # pivot_reciprocal: correctly rounded
                rep.check(np.array_equal(o["x"], s.meta["bitwise"]), r, "1 / d not correctly rounded: %d of %d differ" % (np.sum(o["x"] != s.meta["bitwise"]), s.n))
            if s.family == "zero_rhs":
                rep.check(not np.any(o["x"]), r, "b = 0 gave x != 0")
    rep.finish()


def test_refined_standin_accuracy_and_acceptance(results):
    """Gates (1e8, 1e13) above the fast gate, and (0, 1e13): every system refined."""
    runs, res = results
    rep = Report()
    for r, o in zip(runs, res):
        s = r.system
        if r.form not in C.STANDINS or r.max_ratio_refined == 0:
            continue
        ref = C.system_reference(s)
        if C.expected_plain_verdict(s, ref, r.max_ratio) is not False:
            continue  # accepted unrefined (the plain test), or next to the fast gate
        ratio = s.meta.get("exact_ratio", ref["ratio"])
        refuse = s.meta.get("side") == "refuse" or not ref["pos"] or (ratio > r.max_ratio_refined if "exact_ratio" in s.meta else ratio > r.max_ratio_refined * (1 + C.GATE_MARGIN))
        must = C.must_accept_refined(s, ref) or ("exact_ratio" in s.meta and ratio <= r.max_ratio_refined and ref["refine_ok"])
        if refuse:
            rep.counts["refusal required"] += 1
            rep.check(not o["ok"], r, "accepted where refusal is required (pivot ratio %.17g)" % ratio)
        if must:
            rep.counts["must accept, %s decade %s" % (r.form, C.decade_of(ratio))] += 1
            rep.check(o["ok"], r, "refused on the must-accept set (pivot ratio %.3e, the restated rule accepts after %d corrections)" % (ratio, ref["refine_steps"]))
        if o["ok"] and not refuse:
            rep.counts["refined accepted"] += 1
            xr = ref["x"]
            if not np.any(xr):
                rep.check(not np.any(o["x"]), r, "b = 0 gave x != 0")
                continue
            q = float(np.abs(o["x"] - xr).max() / np.abs(xr).max())
            rep.figure((r.form, s.family, "refined |x - x*| / |x*|"), q)
            rep.check(q <= C.REFINED_TOL, r, "accepted at %.3e |x| from the reference (pivot ratio %.3e)" % (q, ratio))
    rep.finish()


def test_jacobi_and_pivoted_solvers_against_reference(results):
    runs, res = results
    rep = Report()
    paths = collections.Counter()
    for r, o in zip(runs, res):
        s = r.system
        if r.form in C.STANDINS:
            continue
        ref = C.system_reference(s)
        q = C.kappa_error_ratio(s, ref, o["x"])
        rep.figure((r.form, s.family, "error / (n eps kappa |x|)"), q)
        rep.check(q <= C.C_KAPPA, r, "error ratio %.3e > %.3g (kappa %.3e)" % (q, C.C_KAPPA, ref["kappa"]))
        definite = s.kind in ("spd",) or (s.kind == "spectral" and np.all(s.meta["lam"] > 0))
        if definite and r.form in ("eig", "ldlt") and s.kind == "spd":
            qs = C.scaled_error_ratio(s, ref, o["x"])
            rep.figure((r.form, s.family, "scaled error / (n eps kappa_s |x|)"), qs)
            rep.check(qs <= C.C_SCALED, r, "scaled error ratio %.3e > %.3g (kappa_s %.3e)" % (qs, C.C_SCALED, ref["kappa_s"]))
        if "untouched" in s.meta:
            rep.check(not np.any(o["x"][s.meta["untouched"]]), r, "an untouched knot moved")
        if r.form == "eig":
            # The path: preconditioned for positive definite systems; plain for indefinite ones and for semi-definite ones whose
            # zero pivot is exact in floating point too (untouched knots: zero rows and columns).  Where the zero pivot of a
            # semi-definite system is the rounding residue of a cancellation (the dense rank-deficient families: measured, five
            # systems of rank n - 1 or n - 2 came down the preconditioned path) its sign is not the solver's to choose: either path,
            # and the accuracy bound above holds on both.  DESIGN.md states this.
            pre = o["info"] >> 8
            paths[pre] += 1
            rep.counts["eig %s path, %s" % ("preconditioned" if pre else "plain", s.family)] += 1
            if definite:
                rep.check(pre == 1, r, "path bit %d, sweeps %d" % (pre, o["info"] & 255))
            elif s.kind == "general" or "untouched" in s.meta:
                rep.check(pre == 0, r, "path bit %d, sweeps %d" % (pre, o["info"] & 255))
            rep.check(0 < (o["info"] & 255) < 30, r, "%d sweeps" % (o["info"] & 255))
    rep.check(paths[0] > 0 and paths[1] > 0, "all", "eig paths taken: %r" % dict(paths))
    rep.finish()


def test_scaling_by_powers_of_two_changes_no_bit(results):
    runs, res = results
    rep = Report()
    base = {(id(r.system), r.form, r.max_ratio, r.max_ratio_refined): o for r, o in zip(runs, res)}
    for r, o in zip(runs, res):
        s = r.system
        if s.family != "scaled":
            continue
        o0 = base[(id(s.meta["base"]), r.form, r.max_ratio, r.max_ratio_refined)]
        rep.counts["scaled %s" % r.form] += 1
        rep.check(o["ok"] == o0["ok"] and o["info"] == o0["info"], r, "verdict / info %d %d, unscaled %d %d" % (o["ok"], o["info"], o0["ok"], o0["info"]))
        if r.form not in C.STANDINS or o0["ok"]:
            rep.check(np.array_equal(o["x"], o0["x"]), r, "%d entries differ from the unscaled system's" % np.sum(o["x"] != o0["x"]))
    rep.finish()
