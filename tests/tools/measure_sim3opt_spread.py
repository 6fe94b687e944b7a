#!/usr/bin/env python3
"""Measures the tolerance of the OptimizeSim3 tests and writes tests/golden/sim3opt/tolerance.json.  CPU only.

The numeric Jacobian (delta = 1e-9) amplifies 1e-16 differences of the estimate to about 1e-7 in a Jacobian entry, so how far two
correct implementations may end apart is measured, not derived: over every case of tests/optimize_sim3_cases.py the oracle
(tests/optimize_sim3_oracle.py) runs with its edges summed forward and in reverse, and the largest per-entry difference of the
output S12 is taken separately for the quaternion, the translation and the scale.  The bar for product-against-oracle and for
GPU-against-host is FACTOR = 4 times that spread, the margin the solver pins use for two arithmetic variants of one algorithm: it
admits a third variant and not a different iteration count, which moves S12 by orders of magnitude more.

    python tests/tools/measure_sim3opt_spread.py            # writes the file
    python tests/tools/measure_sim3opt_spread.py --check    # recomputes and compares with the file"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import optimize_sim3_cases as sc  # noqa: E402

FACTOR = 4
OUT = os.path.join(os.path.dirname(HERE), "golden", "sim3opt", "tolerance.json")


def measure():
    spread = [0.0, 0.0, 0.0]
    worst = ["", "", ""]
    n = 0
    for name in sorted(sc.cases()):
        for k, (Sf, _, _, Sr) in enumerate(sc.oracle(name)):
            if Sf is None:
                continue
            n += 1
            for j, d in enumerate(sc.diff3(Sf, Sr)):
                if d > spread[j]:
                    spread[j], worst[j] = d, "%s[%d]" % (name, k)
    keys = ("quaternion", "translation", "scale")
    return {"what": "largest per-entry |S12(forward) - S12(reverse)| of tests/optimize_sim3_oracle.py over tests/optimize_sim3_cases.py",
            "script": "tests/tools/measure_sim3opt_spread.py", "problems_with_a_result": n, "factor": FACTOR,
            "spread": dict(zip(keys, spread)), "worst_case": dict(zip(keys, worst)),
            "bar": {k: FACTOR * s for k, s in zip(keys, spread)}}


if __name__ == "__main__":
    got = measure()
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        ok = all(abs(got["spread"][k] - want["spread"][k]) <= 1e-3 * want["spread"][k] for k in got["spread"])
        print(json.dumps(got["spread"]), "matches the file" if ok else "DIFFERS from the file")
        sys.exit(0 if ok else 1)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=2)
        f.write("\n")
    print(json.dumps(got, indent=2))
