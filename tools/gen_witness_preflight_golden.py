#!/usr/bin/env python3
"""Writes tests/golden/witness_preflight_reports.json: status, message and every field of the bp_witness_report that
bp_check_txn_witness gives for every case of tests/witness_preflight_cases.py -- what
tests/test_gpu_witness_preflight_golden.py holds the library to.  Needs a GPU.  Imports only the case lists and the
package's public names, so it runs against the tree it is started in (or the library BPG_LIBBPG names): the committed file
was made from the commit it records.  Every case is run twice and must report the same, and a break must name the rows
that were changed.

    python tools/gen_witness_preflight_golden.py --commit $(git rev-parse HEAD) [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "witness_preflight_reports.json"))
    args = ap.parse_args()
    import txn_table_cases as tc
    import witness_preflight_cases as wc
    from proof_protocol_decoder_amd import proof_gen as pg
    st = tc.build_state(pg)
    out = {"commit": args.commit, "reports": {}}
    try:
        for name, case, words, expect in wc.cases():
            got = wc.report(pg, st, case, words)
            assert got == wc.report(pg, st, case, words), name
            wc.check_expectation(name, got, expect)
            out["reports"][name] = got
            print("%-40s status %d %s" % (name, got["status"], got["message"]))
    finally:
        st.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d reports to %s" % (len(out["reports"]), args.out))


if __name__ == "__main__":
    main()
