"""The inputs whose whole bp_check_txn_witness report is pinned (tests/golden/witness_preflight_reports.json, written by
tools/gen_witness_preflight_golden.py, held by tests/test_gpu_witness_preflight_golden.py): every accepted case of
txn_table_cases.py, and the decoded entry of tests/test_gpu_witness_preflight.py with its own witness and with one cell
of it changed -- each break that file makes, and one of keccak_sponge -> keccak_f.  A plain module.

A changed cell makes a tuple value that one side of a lookup holds and the other does not, which is where the report
does not depend on how unequal non-zero counts of one value are attributed to rows (include/bpg.h, bp_witness_table):
`expect` says which rows the report must name, and the generator holds the recording library to it."""
import txn_table_cases as tc

VERIFY = -5
LOOKUP_FIELDS = ("checked", "holds", "n_looking", "n_looked", "first_looking_row", "first_looked_row")
VIOLATION_FIELDS = ("row", "constraint", "family", "kind", "value")


def _stale_memory_read(w):
    k = next(i for i, r in enumerate(w[6]) if r[0] == 1)
    w[6][k][3] ^= 1
    return dict(match="the witness data given for table memory does not satisfy its AIR", table=6, rows={k - 1, k})


def _broken_sponge_chaining(w):
    k = next(i for i, r in enumerate(w[4]) if r[0] == 1)     # a full block: the next row continues its message
    w[4][k + 1][19 + 3] ^= 1
    return dict(match="the witness data given for table keccak_sponge does not satisfy its AIR", table=4, rows={k, k + 1})


def _another_word(w):
    w[1][0][2] ^= 1                     # byte slot 0 of the first sequence: a valid packing row, but another word
    return dict(match="cross-table lookup byte_packing -> memory does not hold", lookup=1, looking_row=0)


def _another_permutation(w):
    # The Keccak-f table then satisfies its AIR for another input, and the sponge table asks for the original.  Sponge row
    # p absorbs into permutation p (rows 24p .. 24p + 23 of the Keccak-f table, exposed on the last).
    p = 2
    w[3][p][0] ^= 1                     # the low input limb of lane 0
    return dict(match="cross-table lookup keccak_sponge -> keccak_f does not hold", lookup=0, looking_row=p, looked_row=24 * p + 23)


BREAKS = (("decoded_stale_memory_read", _stale_memory_read), ("decoded_broken_sponge_chaining", _broken_sponge_chaining),
          ("decoded_sequence_spells_another_word", _another_word), ("decoded_keccak_input_limb_flipped", _another_permutation))


NAMES = [c.name for c in tc.ACCEPTED] + ["decoded_entry"] + [name for name, _ in BREAKS]


def cases():
    """[(name, case, IR words or None, expect or None)], in NAMES order (decoding the entry takes the library)"""
    out = [(c.name, c, None, None) for c in tc.ACCEPTED]
    good, words = tc.decoded_case()
    out.append((good.name, good, words, None))
    for name, change in BREAKS:
        w = {t: [list(it) for it in items] for t, items in good.witness.items()}
        expect = change(w)
        out.append((name, good._replace(name=name, witness=w), words, expect))
    return out


def as_dict(rc, msg, rep):
    """status, message and every field of a bp_witness_report, as JSON keeps them (viol[]: the n_viol entries; the rest of
    the eight must be zero)"""
    assert all(getattr(v, f) == 0 for t in rep.table for v in t.viol[t.n_viol:] for f in VIOLATION_FIELDS)
    return {"status": rc, "message": msg,
            "table": [{"checked": t.checked, "given": t.given, "n_violated_rows": t.n_violated_rows, "n_viol": t.n_viol,
                       "viol": [{f: getattr(v, f) for f in VIOLATION_FIELDS} for v in t.viol[:t.n_viol]]} for t in rep.table],
            "lookup": [{f: getattr(l, f) for f in LOOKUP_FIELDS} for l in rep.lookup]}


def report(pg, st, case, words):
    return as_dict(*tc.preflight_report(pg, st, case, words))


def check_expectation(name, got, expect):
    """the rows a break's report names are the changed ones.  Only the break of keccak_sponge -> keccak_f may be refused
    instead (the prover's refusal of permutations given beside sponge rows, BP_ERR_INVALID_INPUT): it then names no row."""
    if expect is None:
        assert got["status"] == tc.OK, (name, got["message"])
        return
    if name == "decoded_keccak_input_limb_flipped" and got["status"] == tc.INVALID:
        return
    assert got["status"] == VERIFY, (name, got["status"], got["message"])
    assert expect["match"] in got["message"], (name, got["message"])
    if "table" in expect:
        t = got["table"][expect["table"]]
        rows = {v["row"] for v in t["viol"][:t["n_viol"]]}
        assert rows and rows <= expect["rows"] and t["n_violated_rows"] == len(rows), (name, t)
    else:
        l = got["lookup"][expect["lookup"]]
        assert l["checked"] and not l["holds"] and l["first_looking_row"] == expect["looking_row"], (name, l)
        assert l["first_looked_row"] == expect.get("looked_row", l["first_looked_row"]) and l["first_looked_row"] >= 0, (name, l)
        assert all(t["n_violated_rows"] == 0 for t in got["table"]), name
