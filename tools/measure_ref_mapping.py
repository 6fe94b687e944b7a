"""Re-measures what tests/golden/mapping/tolerance.json records: the spread of x3D from the 4x4 SVD of
src/LocalMapping.cc:331 between the reference's arithmetic variants C and B over the pinned pairs, and the sensitivity figures: how
many frustum points change any bit under variant A instead of C, and how many pairs change under glibc's cosf / atan2f / logf.
Needs the reference tree (make -C oracle/ref mapping measure).

    python tools/measure_ref_mapping.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import ref_mapping as R      # noqa: E402


def main():
    if not R.ensure(variants=("", "_ubsan", "_a", "_b", "_libm")):
        sys.exit("oracle/_ref/ref_mapping and its measurement variants are not built and the reference tree is not present")
    fx = R.load_fixtures()
    tri = [(n, v["req"]) for (k, n), v in sorted(fx.items()) if k == "newpoints"]
    spread, bad, n = R.measure_tri(tri)
    print("x3D of the SVD: spread C / B %.3e over %d pairs -> tolerance %.3e; pairs decided differently: %s" % (spread, n, R.FACTOR * spread, bad or "none"))
    print("recorded: %s" % R.load_tolerance())
    points = changed = 0
    for (k, name), v in sorted(fx.items()):
        if k == "frustum":
            c, a = R.run_ok(v["req"]), R.run_ok(v["req"], "_a")
            diff = np.zeros(c.one("flag").size, bool)
            for tag in ("flag", "level"):
                diff |= (c.one(tag) != a.one(tag)).reshape(-1)
            for tag in ("projx", "projy", "projxr", "viewcos"):
                diff |= (R.bits(c.one(tag)) != R.bits(a.one(tag))).reshape(-1)
            points += diff.size
            changed += int(diff.sum())
    print("frustum: %d of %d points change a bit under variant A instead of C" % (changed, points))
    pairs = changed = 0
    for name, req in tri:
        c, m = R.run_ok(req), R.run_ok(req, "_libm")
        diff = ((c.one("acc") != m.one("acc")) | (c.one("path") != m.one("path"))).reshape(-1) | (R.bits(c.one("x3d")) != R.bits(m.one("x3d"))).any(1)
        pairs += diff.size
        changed += int(diff.sum())
    print("newpoints: %d of %d pairs change under glibc's cosf / atan2f" % (changed, pairs))
    points = changed = 0
    for (k, name), v in sorted(fx.items()):
        if k == "frustum":
            c, m = R.run_ok(v["req"]), R.run_ok(v["req"], "_libm")
            points += c.one("level").size
            changed += int((c.one("level") != m.one("level")).sum() + (c.one("flag") != m.one("flag")).sum())
    print("frustum: %d of %d points change their level under glibc's logf" % (changed, points))


if __name__ == "__main__":
    main()
