#!/usr/bin/env python3
"""Measures the tolerance of the OptimizeEssentialGraph tests and writes tests/golden/eg/tolerance.json.  CPU only.

How far two correct implementations may end apart is measured, not derived.  The numeric Jacobian divides differences of Sim3::log
by 2e-9 and log() calls acos, sin, cos and log on the perturbed values, so one ulp between two math libraries becomes about 1e-7 in
J and moves the Gauss-Newton fixed point by as much; the order of the sums alone moves far less.  Over every case of
tests/eg_cases.py the oracle (tests/eg_oracle.py) runs in six variants, {sums forward, reverse} x {no nudge, every transcendental
+1 ulp, -1 ulp}, and per quantity the largest difference between any two variants is the spread: the entries of the rotations, the
translations t / s, the scales, the corrected points, the final and the initial chi2 (relative).  Left out: the coordinates and the
final chi2 of the GAUGE cases; the ABSOLUTE_CHI2 cases' final chi2 is measured absolutely; the ILL_CONDITIONED case is measured
by itself (eg_cases has the reasons).  The bar for host-against-oracle
and for GPU-against-host is FACTOR = 4 times the spread, this project's margin throughout; it also matches the 4 ulp that OpenCL
conformance allows fp64 acos / sin / cos (the table of the OpenCL C specification, "Relative error as ULPs"), to which the device
library is built, the effect being linear in the ulp error at worst.  No statement of the device library's own bounds was found
beside its sources to cite here.  The product hands poses and points back as floats; the tests add that rounding to the bar
(eg_cases.assert_same).  The spread is never measured against the code under test.

The file also lists the cases whose counts are decided by noise (eg_cases.decisions_clear is False); eg_cases.CONVERGED must name
exactly those.

The scale cases (eg_cases.SCALE_SPECS) are measured the same way, each by itself, into the file's "scale" entry; they take no part
in the common spread.

    python tests/tools/measure_eg_spread.py            # writes the file
    python tests/tools/measure_eg_spread.py --scale     # measures the scale cases alone and puts them into the file as it is
    python tests/tools/measure_eg_spread.py --check     # recomputes and compares with the file"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eg_cases as ec  # noqa: E402

FACTOR = 4


def spread_over(names):
    keys = ec.KEYS + ("chi2_final_absolute",)
    spread, worst = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, "")
    for name in names:
        runs = [ec.oracle(name, *v) for v in ec.VARIANTS]
        for a in range(len(runs)):
            for b in range(a + 1, len(runs)):
                f, r = runs[a], runs[b]
                d = ec.diffs(f["Tcw"], f["Scw"][:, 7], f["xw"], f["stats"]["chi2_final"], f["stats"]["chi2_initial"],
                             r["Tcw"], r["Scw"][:, 7], r["xw"], r["stats"]["chi2_final"], r["stats"]["chi2_initial"])
                d += (abs(f["stats"]["chi2_final"] - r["stats"]["chi2_final"]),)
                for key, x in zip(keys, d):
                    if name in ec.GAUGE and key != "chi2_initial_relative":
                        continue
                    if key == "chi2_final_absolute" and name not in ec.ABSOLUTE_CHI2:
                        continue
                    if key == "chi2_final_relative" and name in ec.ABSOLUTE_CHI2:
                        continue
                    if key == "chi2_initial_relative" and name == "consistent":
                        continue
                    if x > spread[key]:
                        spread[key], worst[key] = x, name
    return {"spread": spread, "worst_case": worst, "bar": {k: FACTOR * s for k, s in spread.items()}}


def measure():
    got = {"what": "largest difference between any two of the six variants (sums forward / reverse x transcendentals nudged by 0, +1, "
                   "-1 ulp) of tests/eg_oracle.py over tests/eg_cases.py",
           "script": "tests/tools/measure_eg_spread.py", "cases": len(ec.NAMES), "factor": FACTOR,
           "device_library_bounds": "none found to cite; the factor equals the 4 ulp OpenCL conformance allows fp64 acos, sin and cos"}
    got.update(spread_over([n for n in ec.NAMES if n not in ec.ILL_CONDITIONED]))
    got["ill_conditioned"] = {n: spread_over([n]) for n in ec.ILL_CONDITIONED}
    got["converged"] = [n for n in ec.NAMES if not ec.decisions_clear(n)]
    got["scale"] = measure_scale()
    return got


def measure_scale():
    """the scale cases, each by itself: a pooled bar would let the small ones hide behind the large ones"""
    for n in ec.SCALE_NAMES:
        assert ec.decisions_clear(n), "%s: a decision of the oracle is not clear of noise" % n
    return {n: spread_over([n]) for n in ec.SCALE_NAMES}


def scale_matches(want, got):
    return (set(want) == set(got) and
            all(want[n]["spread"][k] / FACTOR <= got[n]["spread"][k] <= want[n]["bar"][k] and want[n]["bar"][k] == FACTOR * want[n]["spread"][k]
                for n in got for k in got[n]["spread"]))


if __name__ == "__main__":
    if "--scale" in sys.argv:                   # the scale cases alone, added to the file as it is: every other entry keeps its digits
        want = json.load(open(ec.TOLERANCE))
        want["scale"] = measure_scale()
        with open(ec.TOLERANCE, "w") as f:
            json.dump(want, f, indent=2)
            f.write("\n")
        print(json.dumps(want["scale"], indent=2))
        sys.exit(0)
    got = measure()
    if "--check" in sys.argv:
        want = json.load(open(ec.TOLERANCE))
        if not scale_matches(want.get("scale", {}), got["scale"]):
            print(json.dumps({n: s["spread"] for n, s in got["scale"].items()}), "the scale cases DIFFER from the file")
            sys.exit(1)
        # the oracle's solves go through LAPACK, whose kernels follow the CPU they run on: the recomputed spread must reproduce the
        # recorded one within FACTOR both ways
        ok = (all(want["spread"][k] / FACTOR <= got["spread"][k] <= want["bar"][k] for k in got["spread"])
              and all(want["bar"][k] == FACTOR * want["spread"][k] for k in got["spread"]) and want["factor"] == FACTOR
              and want["converged"] == got["converged"] and set(want["ill_conditioned"]) == set(got["ill_conditioned"]))
        print(json.dumps(got["spread"]), "matches the file" if ok else "DIFFERS from the file")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(ec.TOLERANCE), exist_ok=True)
    with open(ec.TOLERANCE, "w") as f:
        json.dump(got, f, indent=2)
        f.write("\n")
    print(json.dumps(got, indent=2))
