#!/usr/bin/env python3
"""Measures the tolerance of the LocalBundleAdjustment tests and writes tests/golden/lba/tolerance.json.  CPU only.

How far two correct implementations may end apart is measured, not derived: a point that keeps few active edges has a block the
damping alone makes invertible, and the Levenberg factors depend on rho, so rounding differences are amplified by amounts that
depend on the scene.  Over every case of tests/lba_cases.py the oracle (tests/lba_oracle.py) runs with its sums forward and in
reverse, and the largest difference is taken separately for the entries of the pose rotations, the pose translations, the point
coordinates (the cases whose scale is gauge left out) and the final chi2 (relative, every case).  The bar for product-against-oracle
and for GPU-against-host is FACTOR = 4 times that spread, the factor and the reasoning of tests/tools/measure_sim3opt_spread.py: it
admits a third arithmetic variant of one algorithm and not a different trial transcript, which moves the result by orders of
magnitude more.  The product hands poses and points back as floats; the tests add that rounding to the bar (lba_cases.assert_same).

The scale cases (lba_cases.SCALE_NAMES) are measured the same way, each by itself, into the file's "scale" entry; they take no part
in the common spread.

    python tests/tools/measure_lba_spread.py            # writes the file
    python tests/tools/measure_lba_spread.py --scale    # measures the scale cases alone and puts them into the file as it is
    python tests/tools/measure_lba_spread.py --check    # recomputes and compares with the file"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lba_cases as lc  # noqa: E402

FACTOR = 4
OUT = os.path.join(os.path.dirname(HERE), "golden", "lba", "tolerance.json")


def spread_over(names):
    spread = [0.0] * 4
    worst = [""] * 4
    for name in names:
        f, r = lc.oracle(name)
        d = lc.diffs(f["Tcw"], f["xw"], f["stats"]["chi2"], r["Tcw"], r["xw"], r["stats"]["chi2"])
        for j, x in enumerate(d):
            if j < 3 and name in lc.GAUGE:
                continue
            if x > spread[j]:
                spread[j], worst[j] = x, name
    return {"spread": dict(zip(lc.KEYS, spread)), "worst_case": dict(zip(lc.KEYS, worst)),
            "bar": {k: FACTOR * s for k, s in zip(lc.KEYS, spread)}}


def measure_scale():
    """the scale cases, each by itself: a pooled bar would let the small ones hide behind the large ones"""
    return {n: spread_over([n]) for n in lc.SCALE_NAMES}


def scale_matches(want, got):
    return (set(want) == set(got) and
            all(want[n]["spread"][k] / FACTOR <= got[n]["spread"][k] <= want[n]["bar"][k] and want[n]["bar"][k] == FACTOR * want[n]["spread"][k]
                for n in got for k in got[n]["spread"]))


def measure():
    got = {"what": "largest |forward - reverse| of tests/lba_oracle.py over tests/lba_cases.py",
           "script": "tests/tools/measure_lba_spread.py", "cases": len(lc.NAMES), "factor": FACTOR}
    got.update(spread_over(lc.NAMES))
    got["scale"] = measure_scale()
    return got


if __name__ == "__main__":
    if "--scale" in sys.argv:                   # the scale cases alone, added to the file as it is: every other entry keeps its digits
        want = json.load(open(OUT))
        want["scale"] = measure_scale()
        with open(OUT, "w") as f:
            json.dump(want, f, indent=2)
            f.write("\n")
        print(json.dumps(want["scale"], indent=2))
        sys.exit(0)
    got = measure()
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        if not scale_matches(want.get("scale", {}), got["scale"]):
            print(json.dumps({n: s["spread"] for n, s in got["scale"].items()}), "the scale cases DIFFER from the file")
            sys.exit(1)
        # the oracle's Schur product and its solve go through BLAS / LAPACK, whose kernels and blocking follow the CPU they run on:
        # the recomputed spread need not equal the file's last digits, but it must reproduce the recorded one within FACTOR both
        # ways: at most the file's bar, and at least recorded / FACTOR, so that a file whose spread is too large fails as well
        ok = (all(want["spread"][k] / FACTOR <= got["spread"][k] <= want["bar"][k] for k in got["spread"])
              and all(want["bar"][k] == FACTOR * want["spread"][k] for k in got["spread"]) and want["factor"] == FACTOR)
        print(json.dumps(got["spread"]), "matches the file" if ok else "DIFFERS from the file")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=2)
        f.write("\n")
    print(json.dumps(got, indent=2))
