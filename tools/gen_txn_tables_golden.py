#!/usr/bin/env python3
"""Writes tests/golden/txn_tables_digests.json: sha256 of the table proofs of every accepted case of
tests/txn_table_cases.py (and of the decoded entry), and of the whole transaction proof of one of them -- what
tests/test_gpu_txn_tables.py holds the library to.  Needs a GPU.  Imports only the case list and the package's public
names, so it runs against the tree it is started in: the committed file was made from the commit it records.

    python tools/gen_txn_tables_golden.py --commit $(git rev-parse HEAD) [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "txn_tables_digests.json"))
    args = ap.parse_args()
    import txn_table_cases as tc
    from proof_protocol_decoder_amd import proof_gen as pg
    st = tc.build_state(pg)
    out = {"commit": args.commit, "table_proofs": {}, "txn_proof": {}}
    try:
        for case, words in [(c, None) for c in tc.ACCEPTED] + [tc.decoded_case()]:
            rc, msg, blob = tc.table_proofs(pg, st, case, words)
            assert rc == 0, (case.name, msg)
            out["table_proofs"][case.name] = hashlib.sha256(blob).hexdigest()
            if case.name == tc.FULL_PROOF:
                rc, msg, blob = tc.txn_proof(pg, st, case, words)
                assert rc == 0, (case.name, msg)
                out["txn_proof"][case.name] = hashlib.sha256(blob).hexdigest()
    finally:
        st.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(out["table_proofs"]) + len(out["txn_proof"]), args.out))


if __name__ == "__main__":
    main()
