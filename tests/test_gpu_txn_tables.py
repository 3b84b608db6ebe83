"""The cases of txn_table_cases.py on the device: a refused case is refused alike, status and message, by the pre-flight
and by the prover; an accepted case gives table proofs whose sha256 is the one tests/golden/txn_tables_digests.json
records (tools/gen_txn_tables_golden.py wrote it from the commit it names: no byte of a proof moves without that file
moving), and one case the whole transaction proof."""
import hashlib
import json
import os
import time

import pytest

import txn_table_cases as tc

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txn_tables_digests.json")))


@pytest.fixture(scope="module")
def prover(bpg):
    from proof_protocol_decoder_amd import proof_gen as pg
    st = tc.build_state(pg)
    yield pg, st
    st.close()


@pytest.mark.parametrize("case", tc.REFUSED, ids=lambda c: c.name)
def test_a_refused_case_is_refused_alike_by_the_preflight_and_the_prover(prover, case):
    pg, st = prover
    rc, msg = tc.preflight(pg, st, case)
    assert rc == case.status and case.match in msg, (rc, msg)
    rc, msg, _ = tc.table_proofs(pg, st, case)
    assert rc == case.status and case.match in msg, (rc, msg)


@pytest.mark.parametrize("case", tc.ACCEPTED, ids=lambda c: c.name)
def test_the_table_proofs_of_an_accepted_case_are_the_recorded_bytes(prover, case):
    pg, st = prover
    rc, msg, blob = tc.table_proofs(pg, st, case)
    assert rc == tc.OK, msg
    assert hashlib.sha256(blob).hexdigest() == GOLDEN["table_proofs"][case.name]


def test_the_decoded_entry_with_its_own_witness(prover):
    pg, st = prover
    case, words = tc.decoded_case()
    rc, msg = tc.preflight(pg, st, case, words)
    assert rc == tc.OK, msg
    rc, msg, blob = tc.table_proofs(pg, st, case, words)
    assert rc == tc.OK, msg
    assert hashlib.sha256(blob).hexdigest() == GOLDEN["table_proofs"][case.name]


def test_a_whole_transaction_proof_is_the_recorded_bytes(prover):
    pg, st = prover
    case = next(c for c in tc.ACCEPTED if c.name == tc.FULL_PROOF)
    t0 = time.perf_counter()
    rc, msg, blob = tc.txn_proof(pg, st, case)
    print("lone transaction (%s): %.1f ms" % (case.name, 1e3 * (time.perf_counter() - t0)))
    assert rc == tc.OK, msg
    assert hashlib.sha256(blob).hexdigest() == GOLDEN["txn_proof"][case.name]
