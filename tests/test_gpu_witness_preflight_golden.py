"""bp_check_txn_witness against the reports tests/golden/witness_preflight_reports.json records
(tools/gen_witness_preflight_golden.py wrote it from the commit it names): status, message and every field of the report
of every case of witness_preflight_cases.py.  Each case is run twice: the report is a function of the inputs, not of the
call's challenges."""
import json
import os

import pytest

import txn_table_cases as tc
import witness_preflight_cases as wc

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "witness_preflight_reports.json")))


@pytest.fixture(scope="module")
def prover(bpg):
    from proof_protocol_decoder_amd import proof_gen as pg
    st = tc.build_state(pg)
    yield pg, st, {name: rest for name, *rest in wc.cases()}
    st.close()


def test_every_case_is_recorded(prover):
    assert sorted(GOLDEN["reports"]) == sorted(wc.NAMES) == sorted(prover[2])


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_report_is_the_recorded_one(prover, name):
    pg, st, cases = prover
    case, words, expect = cases[name]
    got = wc.report(pg, st, case, words)
    want = GOLDEN["reports"][name]
    assert got["status"] == want["status"] and got["message"] == want["message"]
    for t in range(7):
        assert got["table"][t] == want["table"][t], ("table", t)
    for i in range(3):
        assert got["lookup"][i] == want["lookup"][i], ("lookup", i)
    assert got == wc.report(pg, st, case, words)
    wc.check_expectation(name, got, expect)
