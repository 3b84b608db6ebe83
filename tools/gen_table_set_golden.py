#!/usr/bin/env python3
"""Writes tests/golden/table_set_digests.json: sha256 and length of the "BPGTSET1" container of every set of
tests/air_program_port_cases.py's table_set_byte_cases -- what tests/test_gpu_table_set_bytes.py holds
bp_stark_prove_table_set to.  Needs a GPU.  Goes through the package's ops only, so it runs against the library of the
tree it is started in (or the one BPG_LIBBPG names): the committed file was made from the commit it records.

    python tools/gen_table_set_golden.py --commit $(git rev-parse HEAD) [--out FILE] [--containers DIR]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digests(bpg, keep=None):
    """{name: {"sha256", "bytes"}} of the byte cases' containers; keep (a dict) receives the containers themselves"""
    import air_program_port_cases as pc
    out = {}
    for name, (tables, links) in pc.table_set_byte_cases(bpg).items():
        raw = bpg.ops.stark_prove_table_set(tables, links).tobytes()
        out[name] = {"sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw)}
        if keep is not None:
            keep[name] = raw
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "table_set_digests.json"))
    ap.add_argument("--containers", help="a directory that receives every container as <name>.bin")
    args = ap.parse_args()
    import proof_protocol_decoder_amd as bpg
    bpg.lib()
    keep = {}
    out = {"commit": args.commit, "containers": digests(bpg, keep)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.containers:
        os.makedirs(args.containers, exist_ok=True)
        for name, raw in keep.items():
            with open(os.path.join(args.containers, name + ".bin"), "wb") as f:
                f.write(raw)
    print("wrote %d digests to %s" % (len(out["containers"]), args.out))


if __name__ == "__main__":
    main()
