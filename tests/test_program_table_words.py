"""The assembled words of the shipped tables' programs, by SHA-256 (tests/golden/program_table_words.json): a program's
registered id is a digest of its words and the K5 timings of DESIGN.md section 7 belong to them, so a change to
word_table.py, arithmetic_div.py or arithmetic_mod.py that reorders the Builder's operations shows here.  A deliberate
change to a program updates the file in the same commit."""
import hashlib
import json
import os

import pytest

from proof_protocol_decoder_amd import arithmetic_div, arithmetic_mod

with open(os.path.join(os.path.dirname(__file__), "golden", "program_table_words.json")) as f:
    GOLDEN = json.load(f)
PROGRAMS = {"division": arithmetic_div.program, "modular": arithmetic_mod.program}
CASES = [(table, int(units)) for table in ("division", "modular") for units in GOLDEN[table]]


def test_the_file_holds_the_eight_programs():
    assert CASES == [("division", u) for u in (1, 2, 4, 8, 16)] + [("modular", u) for u in (1, 2, 4)]


@pytest.mark.parametrize("table,units", CASES, ids=["%s-%d" % c for c in CASES])
def test_the_assembled_words_are_the_recorded_ones(table, units):
    words = PROGRAMS[table](units).assemble()
    assert hashlib.sha256(words.tobytes()).hexdigest() == GOLDEN[table][str(units)]
