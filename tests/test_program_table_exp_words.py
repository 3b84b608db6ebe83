"""The assembled words of the exponentiation table's program, by SHA-256 (tests/golden/program_table_exp_words.json), one
digest per unit cut program() accepts: the registered id is a digest of the words and the K5 timings of DESIGN.md section
7 belong to them, so a change to word_table.py or arithmetic_exp.py that reorders the Builder's operations shows here
(tests/test_program_table_words.py, tests/test_program_table_shift_words.py and tests/test_program_table_sdiv_words.py
hold the other four tables).  A deliberate change to the program updates the file in the same commit."""
import hashlib
import json
import os

import pytest

from proof_protocol_decoder_amd import arithmetic_exp

with open(os.path.join(os.path.dirname(__file__), "golden", "program_table_exp_words.json")) as f:
    GOLDEN = json.load(f)


def test_the_file_holds_one_digest_per_cut():
    assert [int(c) for c in GOLDEN["exp"]] == list(arithmetic_exp.CUTS) == [1, 2, 4]
    assert arithmetic_exp.LIMBS_PER_UNIT in arithmetic_exp.CUTS


@pytest.mark.parametrize("cut", arithmetic_exp.CUTS)
def test_the_assembled_words_are_the_recorded_ones(cut):
    words = arithmetic_exp.program(cut).assemble()
    assert hashlib.sha256(words.tobytes()).hexdigest() == GOLDEN["exp"][str(cut)]
