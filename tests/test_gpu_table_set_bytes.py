"""The bytes of a table-set proof: the "BPGTSET1" containers of tests/air_program_port_cases.py's four byte cases have
the sha256 and the length tests/golden/table_set_digests.json records (tools/gen_table_set_golden.py wrote it from the
commit it names).  The other set tests prove and verify, which a reordered observe would survive: the prover and the
verifier would move together and the statement's transcript would change unnoticed.  Here no byte moves without that file."""
import hashlib
import json
import os

import pytest

import air_program_port_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_set_digests.json")))["containers"]
CASES = ["a_product_link_strided", "b_two_looking_tables", "c_log_range_self_link", "d_into_built_in_memory"]


@pytest.fixture(scope="module")
def sets(bpg):
    return pc.table_set_byte_cases(bpg)


def test_the_fixture_holds_the_four_cases():
    assert sorted(GOLDEN) == CASES


@pytest.mark.parametrize("name", CASES)
def test_a_table_sets_container_is_byte_for_byte_the_recorded_one(bpg, sets, name):
    tables, links = sets[name]
    raw = bpg.ops.stark_prove_table_set(tables, links).tobytes()
    assert len(raw) == GOLDEN[name]["bytes"]
    assert hashlib.sha256(raw).hexdigest() == GOLDEN[name]["sha256"]
    if name == "a_product_link_strided":    # the second member is a column slice: the pack is on the path
        assert tables[1]["trace"].stride(0) == tables[1]["trace"].shape[1] + 3
