"""The assembled words of the five shipped tables' programs, by SHA-256 (tests/golden/program_table_words.json), one
digest per unit cut program() accepts: a program's registered id is a digest of its words and the K5 timings of DESIGN.md
section 7 belong to them, so a change to word_table.py or to a table's module that reorders the Builder's operations
shows here.  A deliberate change to a program updates the file in the same commit."""
import hashlib
import json
import os

import pytest

from proof_protocol_decoder_amd import arithmetic_div, arithmetic_exp, arithmetic_mod, arithmetic_sdiv, arithmetic_shift

with open(os.path.join(os.path.dirname(__file__), "golden", "program_table_words.json")) as f:
    GOLDEN = json.load(f)
MODULES = {"division": arithmetic_div, "modular": arithmetic_mod, "shift": arithmetic_shift, "sdiv": arithmetic_sdiv,
           "exp": arithmetic_exp}
CASES = [(table, int(cut)) for table in GOLDEN for cut in GOLDEN[table]]


def test_the_file_holds_the_sixteen_programs():
    cuts = {"division": (1, 2, 4, 8, 16), "modular": (1, 2, 4), "shift": (1, 2, 4), "sdiv": (1, 2), "exp": (1, 2, 4)}
    assert CASES == [(table, cut) for table in MODULES for cut in cuts[table]] and len(CASES) == 16
    for table in ("shift", "sdiv", "exp"):   # the modules that state their cuts
        assert MODULES[table].CUTS == cuts[table] and MODULES[table].LIMBS_PER_UNIT in cuts[table]


@pytest.mark.parametrize("table,cut", CASES, ids=["%s-%d" % c for c in CASES])
def test_the_assembled_words_are_the_recorded_ones(table, cut):
    words = MODULES[table].program(cut).assemble()
    assert hashlib.sha256(words.tobytes()).hexdigest() == GOLDEN[table][str(cut)]
