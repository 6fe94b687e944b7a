"""Record tests/golden/matcher/*.npz: the requests of ref_matcher.fixture_cases() and the responses of the pin
(oracle/_ref/ref_matcher, the reference's own src/ORBmatcher.cc on the shim's arithmetic variant C), as byte arrays.

    make -C oracle/ref matcher measure && python tests/golden/make_golden_matcher.py

Every planted case must agree between the pin and variant A (oracle/_ref/ref_matcher_a) in every compared field, or nothing is
written.  A file holds "<case>_req" and "<case>_rsp"; files are split so that none exceeds LIMIT bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (makes the package importable)
import ref_matcher as R  # noqa: E402

LIMIT = 112 * 1024          # below the largest fixture of tests/golden/solvers (init.npz)


def main():
    assert R.have_binary() and R.have_binary("_a"), "make -C oracle/ref matcher measure"
    groups = {}
    for case in R.fixture_cases():
        out, rec = R.ask_case(case, "binary")
        if case.planted:
            out_a, _ = R.ask_case(case, "binary", "_a")
            assert R.same(out, out_a), "variant A and the pin differ on the planted case %s" % case.name
        prefix = case.name.split("-")[0] + "-" + case.kind
        groups.setdefault(prefix, []).append((case.name, rec.request, rec.data))
    for old in os.listdir(R.GOLDEN):
        if old.endswith(".npz"):
            os.remove(os.path.join(R.GOLDEN, old))
    for prefix, items in sorted(groups.items()):
        part, held, size = 0, {}, 0

        def flush():
            nonlocal part, held, size
            if held:
                path = os.path.join(R.GOLDEN, "%s-%d.npz" % (prefix, part))
                np.savez_compressed(path, **held)
                assert os.path.getsize(path) <= 118162, (path, os.path.getsize(path))
                print("%-28s %3d cases %7d bytes" % (os.path.basename(path), len(held) // 2, os.path.getsize(path)))
                part, held, size = part + 1, {}, 0

        for name, rq, rs in items:
            if size + len(rq) + len(rs) // 3 > LIMIT:
                flush()
            held[name + "_req"] = np.frombuffer(rq, np.uint8)
            held[name + "_rsp"] = np.frombuffer(rs, np.uint8)
            size += len(rq) + len(rs) // 3
        flush()


if __name__ == "__main__":
    main()
