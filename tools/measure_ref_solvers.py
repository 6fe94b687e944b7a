#!/usr/bin/env python3
"""Re-measures the spreads between the two arithmetic variants of the solvers' reference pin and, with
--record, rewrites the fixtures under tests/golden/solvers/ from variant A.

    make -C oracle/ref solvers measure        # ref_sim3 / ref_pnp / ref_init, their UBSan copies and their B variants
    python tools/measure_ref_solvers.py [--record]

Prints one line per compared quantity: the measured spread, the constant in tests/ref_solvers.py and the tolerance (4 x the
constant).  Fails when the two variants disagree on an exactly compared field of a pinned case (such a case has to be replaced), or
when a measured spread is above its constant."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_solvers as rs  # noqa: E402


def main():
    spreads = rs.record_fixtures() if "--record" in sys.argv[1:] else None
    if spreads is None:
        spreads, disagreements = rs.measure_spreads()
        if disagreements:
            print("the variants disagree on exact fields:", disagreements)
            return 1
    bad = 0
    for q in sorted(rs.SPREADS):
        m = spreads.get(q, 0.0)
        print("%-14s measured %.3e   constant %.1e   tolerance %.1e%s" % (q, m, rs.SPREADS[q], rs.tol(q), "   ABOVE THE CONSTANT" if m > rs.SPREADS[q] else ""))
        bad += m > rs.SPREADS[q]
    if spreads is not None and "--record" in sys.argv[1:]:
        for kind in rs.KINDS:
            print("wrote %s (%d bytes)" % (os.path.relpath(rs.fixture_path(kind), ROOT), os.path.getsize(rs.fixture_path(kind))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
