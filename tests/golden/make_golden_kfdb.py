"""Regenerates tests/golden/kfdb/: two case scripts of tests/ref_kfdb.py and the output oracle/_ref/ref_kfdb (the
reference's own src/KeyFrameDatabase.cc) gives for them.  Data only: the scripts are this project's, the outputs are
candidate ids, lScoreAndMatch entries and key-frame fields.  Needs the reference tree (make -C oracle/ref kfdb).

    python tests/golden/make_golden_kfdb.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ref_kfdb as R      # noqa: E402


def golden_cases():
    # small on purpose: a 100-operation sequence over 12 key frames with two dumps; the second-chunk and last-entry groups
    # of the chunk case at 0, 65 and 129 entries
    return {"control": R.case_random(11, nops=100, nkf=12, dump_every=50),
            "edges": R.case_chunks(lengths=(0, 65, 129), only=("second_chunk", "last_entry"))}


def main():
    if R.ensure() is None:
        sys.exit("oracle/_ref/ref_kfdb is not built and the reference tree is not present")
    os.makedirs(R.GOLDEN, exist_ok=True)
    for name, c in golden_cases().items():
        out = R.run_ref_text(c.text)
        ev = R.parse_output(out)
        if c.proof:
            c.proof(ev)
        assert R.run_ref_text(c.text, R.EXE_UBSAN) == out
        with open(os.path.join(R.GOLDEN, name + ".script"), "w") as f:
            f.write(c.text)
        with open(os.path.join(R.GOLDEN, name + ".out"), "w") as f:
            f.write(out)
        print("%s: %d queries, script %d bytes, output %d bytes" % (name, c.nqueries, len(c.text), len(out)))


if __name__ == "__main__":
    main()
